"""crawford_item4_kernel in its DPP form (csrc/crawford.hip, BSP_CW_BCAST=1), checked without a GPU: the resources its occupancy
rests on, from the code-object notes, and the wait states of its hand-written DPP instructions, from the assembly.

The compiler pads nothing inside an asm statement.  A DPP instruction must not read, as its DPP source, a VGPR that a VALU
instruction wrote fewer than 2 wait states earlier, nor follow a VALU write of EXEC by fewer than 5 (LLVM's GCNHazardRecognizer:
DppVgprWaitStates = 2, DppExecWaitStates = 5).  An instruction is one wait state, `s_nop N` is N + 1."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bspatom_amd", "csrc")

WAVES_PER_SIMD = 4                       # the occupancy the DPP form ships with
VGPR_CAP = 512 // WAVES_PER_SIMD         # gfx950: 512 VGPRs per SIMD lane
LDS_PER_WAVE = 160 * 1024 // (4 * WAVES_PER_SIMD)   # 160 KiB per CU, four SIMDs


def test_resources_of_the_dpp_instances():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    inst = {n: v for n, v in ks.items() if "crawford_item4_kernel<" in n and n.rstrip().endswith("true>")}
    assert len(inst) == 3, sorted(inst)                              # <false, 1>, <false, 4>, <true, 1>
    for name, v in inst.items():
        nw = v["max_flat_workgroup_size"] // 64
        print(name, v)
        assert not v["private_segment_fixed_size"] and not v["vgpr_spill_count"] and not v["sgpr_spill_count"], (name, v)
        assert v["vgpr_count"] + (v["agpr_count"] or 0) <= VGPR_CAP, (name, v)
        assert v["group_segment_fixed_size"] <= nw * LDS_PER_WAVE, (name, v)


def _assembly(tmp_path):
    """crawford.hip's device assembly under the Makefile's own command for build/crawford.o"""
    cmds = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/crawford.o"], text=True).splitlines()
    cmd = [c for c in cmds if "crawford.hip" in c and " -c " in c]
    assert len(cmd) == 1, cmds
    out = str(tmp_path / "crawford.s")
    words = cmd[0].split()
    words = words[:words.index("-o")] + ["-o", out]
    words[words.index("-c")] = "-S"
    subprocess.check_call(words + ["--cuda-device-only", "-w"], cwd=CSRC)
    return open(out).read().splitlines()


def _regs(op):
    """VGPR numbers an operand names: 'v[40:41]' -> {40, 41}, 'v7' -> {7}, anything else -> {}"""
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", op)
    return {int(m.group(1))} if m else set()


def _parse(line):
    """(mnemonic, [operands]) of an instruction line, None for labels, directives, comments"""
    s = line.split(";")[0].strip()
    if not s or s.startswith(".") or s.endswith(":"):
        return None
    mn, _, rest = s.partition(" ")
    return mn, [o.strip().split(" ")[0] for o in rest.split(",")] if rest else []


def _vgprs_written(mn, ops):
    if not mn.startswith("v_") or not ops:
        return set()
    if mn.startswith("v_swap"):
        return _regs(ops[0]) | _regs(ops[1])
    return _regs(ops[0])


def _writes_exec(mn, ops):
    return mn.startswith("v_cmpx") or (mn.startswith("v_") and bool(ops) and ops[0].startswith("exec"))


def hazards(lines):
    """[(line number, text, why)] of every DPP instruction with a producer inside its wait states; also the number of DPP instructions"""
    bad, ndpp = [], 0
    prog = []                                                           # (line number, parsed or "label")
    for i, line in enumerate(lines):
        s = line.split(";")[0].strip()
        if s.endswith(":") and not s.startswith("."):
            prog.append((i + 1, "label"))
            continue
        p = _parse(line)
        if p:
            prog.append((i + 1, p))
    for at, (ln, p) in enumerate(prog):
        if p == "label" or "_dpp" not in p[0]:
            continue
        ndpp += 1
        src = _regs(p[1][1])
        assert src, (ln, p)
        states = 0
        for ln2, q in reversed(prog[:at]):
            if states >= 5:
                break
            if q == "label":
                if states < 2:
                    bad.append((ln, lines[ln - 1].strip(), "a label %d states before: the producers are not all in sight" % states))
                break
            mn, ops = q
            if mn == "s_nop":
                states += int(ops[0], 0) + 1
                continue
            if states < 2 and _vgprs_written(mn, ops) & src:
                bad.append((ln, lines[ln - 1].strip(), "DPP source written %d states before, line %d: %s" % (states, ln2, lines[ln2 - 1].strip())))
            if _writes_exec(mn, ops):
                bad.append((ln, lines[ln - 1].strip(), "EXEC written %d states before, line %d" % (states, ln2)))
            states += 1
    return bad, ndpp


def test_the_walker_sees_a_hazard():
    ok = ["\tv_mul_f64 v[2:3], v[4:5], v[6:7]", "\ts_nop 1", "\tv_fmac_f64_dpp v[8:9], v[2:3], v[4:5] row_newbcast:3 row_mask:0xf bank_mask:0xf"]
    assert hazards(ok) == ([], 1)
    for body in (["\tv_mul_f64 v[2:3], v[4:5], v[6:7]"],                               # no state in between
                 ["\tv_mul_f64 v[2:3], v[4:5], v[6:7]", "\ts_nop 0"],                   # one
                 ["\tv_mov_b32_e32 v3, v1", "\tv_add_f64 v[10:11], v[4:5], v[6:7]"],    # half of the pair, one instruction between
                 ["\tv_cmpx_lt_f64_e32 v[4:5], v[6:7]", "\ts_nop 2", "\tv_nop"]):       # EXEC four states before
        bad, n = hazards(body + [ok[2]])
        assert n == 1 and len(bad) == 1, (body, bad)
    two = ["\tv_mul_f64 v[2:3], v[4:5], v[6:7]", "\tv_add_f64 v[10:11], v[4:5], v[6:7]", "\tv_add_f64 v[12:13], v[4:5], v[6:7]", ok[2]]
    assert hazards(two) == ([], 1)                                                      # two independent instructions are two states


def test_no_dpp_instruction_inside_its_wait_states(tmp_path):
    lines = _assembly(tmp_path)
    bad, ndpp = hazards(lines)
    n64 = sum(1 for l in lines if "v_fmac_f64_dpp" in l or "v_mov_b64_dpp" in l)
    print("%d DPP instructions, %d of them 64-bit" % (ndpp, n64))
    # three instances; step I has four loops of 9 + I FMAs and two moves; the last step's update of the F part of X is dead code,
    # and the two-division form updates q[LEN] outside the statements
    assert n64 >= 3 * (sum(4 * (9 + i) + 2 for i in range(8)) - 8) - 2 * 8, n64
    assert not bad, bad[:10]
