"""The chase on tiles of 8 with the reflector and z as DPP operands of its FMAs (csrc/sbr2.hip, BSP_SBR_XDPP), checked without a GPU:
the wait states of its hand-written DPP instructions, from the assembly, and the resources of its instances, from the code-object
notes.

The rule and the walker are those of test_host_cw_codeobj.py (a DPP source is read no sooner than 2 wait states after a VALU write
of it, 5 after a VALU write of EXEC).  The hand-written instructions are the ones with row_newbcast: the compiler forms none, and
pads its own DPP instructions (the row sums) itself.  These carry a bank mask (an item is half a DPP row), and a masked DPP
instruction also READS ITS DESTINATION by the same path: the lanes the mask leaves out are written back with it.  Directly behind
an instruction that wrote the accumulator it puts the accumulator's old value back (measured, profiles/r24_chase8_dpp.txt), so the
same 2 wait states are asked of the destination here."""
import os
import re
import subprocess
import sys

from test_host_cw_codeobj import CSRC, ROOT, VGPR_CAP, _parse, _regs, _vgprs_written, hazards


def masked_destination_hazards(lines):
    """[(line number, text, why)] of every masked row_newbcast instruction whose destination a VALU instruction (another DPP one
    included) wrote fewer than 2 wait states earlier, or which has a label that close in front of it"""
    bad = []
    prog = []
    for i, line in enumerate(lines):
        t = line.split(";")[0].strip()
        if t.endswith(":") and not t.startswith("."):
            prog.append((i + 1, "label"))
        elif _parse(line):
            prog.append((i + 1, _parse(line)))
    for at, (ln, p) in enumerate(prog):
        if p == "label" or "_dpp" not in p[0] or "row_newbcast" not in lines[ln - 1] or "bank_mask:0xf" in lines[ln - 1]:
            continue
        dst = _regs(p[1][0])
        assert dst, (ln, p)
        states = 0
        for ln2, q in reversed(prog[:at]):
            if states >= 2:
                break
            if q == "label":
                bad.append((ln, lines[ln - 1].strip(), "a label %d states before" % states))
                break
            mn, ops = q
            if mn == "s_nop":
                states += int(ops[0], 0) + 1
                continue
            if _vgprs_written(mn, ops) & dst:
                bad.append((ln, lines[ln - 1].strip(), "destination written %d states before, line %d: %s" % (states, ln2, lines[ln2 - 1].strip())))
            states += 1
    return bad


def test_the_walker_sees_a_masked_destination_hazard():
    lo = "\tv_fmac_f64_dpp v[8:9], v[2:3], v[4:5] row_newbcast:3 row_mask:0xf bank_mask:0x3"
    hi = "\tv_fmac_f64_dpp v[8:9], v[2:3], v[4:5] row_newbcast:11 row_mask:0xf bank_mask:0xc"
    other = "\tv_fmac_f64_dpp v[10:11], v[2:3], v[4:5] row_newbcast:3 row_mask:0xf bank_mask:0x3"
    assert len(masked_destination_hazards(["\ts_nop 1", lo, hi])) == 1                    # the pair as neighbours
    assert len(masked_destination_hazards(["\ts_nop 1", lo, other, hi])) == 1            # one instruction between
    assert masked_destination_hazards(["\ts_nop 1", lo, other, other.replace("v[10:11]", "v[12:13]"), hi]) == []
    assert len(masked_destination_hazards(["\tv_mov_b32_e32 v9, v1", "\ts_nop 0", lo])) == 1
    assert masked_destination_hazards(["\tv_mov_b32_e32 v9, v1", "\ts_nop 1", lo]) == []


def _assembly(tmp_path):
    """sbr2.hip's device assembly under the Makefile's own command for build/sbr2.o"""
    cmds = subprocess.check_output(["make", "-n", "-B", "-C", CSRC, "build/sbr2.o"], text=True).splitlines()
    cmd = [c for c in cmds if "sbr2.hip" in c and " -c " in c]
    assert len(cmd) == 1, cmds
    out = str(tmp_path / "sbr2.s")
    words = cmd[0].split()
    words = words[:words.index("-o")] + ["-o", out]
    words[words.index("-c")] = "-S"
    subprocess.check_call(words + ["--cuda-device-only", "-w"], cwd=CSRC)
    return open(out).read().splitlines()


def test_no_hand_written_dpp_instruction_inside_its_wait_states(tmp_path):
    lines = _assembly(tmp_path)
    bad, ndpp = hazards(lines)
    ours = [l for l in lines if "row_newbcast" in l]
    assert all("v_fmac_f64_dpp" in l for l in ours), [l for l in ours if "v_fmac_f64_dpp" not in l][:5]
    # an item is half a DPP row: every broadcast is a pair, lanes 0 .. 7 from lane i and lanes 8 .. 15 from lane 8 + i
    lo = sum(1 for l in ours if re.search(r"row_newbcast:[0-7] row_mask:0xf bank_mask:0x3", l))
    hi = sum(1 for l in ours if re.search(r"row_newbcast:([89]|1[0-5]) row_mask:0xf bank_mask:0xc", l))
    print("%d DPP instructions, %d of them hand-written (%d + %d)" % (ndpp, len(ours), lo, hi))
    assert lo == hi and lo + hi == len(ours)
    # per step and instance (plain, instrumented): setting 1: 8 pairs in role 1; setting 2: 7 + 16; setting 3: that, 7 + 7 in role 0 and
    # 7 + 8 in role 2.  Every role's step stands in the code at least once (general body), the steady bodies add more
    assert lo >= 2 * (8 + 23 + 23 + 14 + 15), lo
    badd = masked_destination_hazards(lines)
    assert not badd, badd[:10]
    bad = [b for b in bad if "row_newbcast" in b[1]]
    assert not bad, bad[:10]


def test_resources_of_the_tiles_of_8_instances():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    ks = codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))
    inst = {n: v for n, v in ks.items() if "sbr_rows_kernel<8," in n or "sbr_rows_xdpp_kernel<" in n or "sbr_rows_general_kernel<8," in n}
    # the default setting (plain, instrumented), the three other settings of each, the general loop of each
    assert len(inst) == 2 + 6 + 2, sorted(inst)
    assert sum(1 for n in inst if "sbr_rows_kernel<8, false>" in n) == 1, sorted(inst)       # what runs by default
    for name, v in inst.items():
        print(name, v)
        # two workgroups of seven waves per CU: four waves per SIMD.  (Scalar registers do spill, into lanes of a vector register
        # that is counted below: no memory behind them.)
        assert not v["private_segment_fixed_size"] and not v["vgpr_spill_count"], (name, v)
        assert v["vgpr_count"] + (v["agpr_count"] or 0) <= VGPR_CAP, (name, v)
