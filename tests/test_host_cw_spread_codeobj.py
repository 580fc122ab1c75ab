"""crawford_item4_spread_kernel (csrc/crawford.hip, BSP_CW_SPREAD), checked without a GPU from the code-object notes: no scratch,
registers for four waves per SIMD, a workgroup of SPREAD waves; and the one-wave instances of the DPP form, which the spread
parameter must leave as they were."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# crawford_item4_kernel<ONEDIV, NW, true> in the build of the commit before cw_quad took its SPREAD parameter: (VGPRs, bytes of LDS)
BEFORE = {"bsp::crawford_item4_kernel<false, 1, true>": (120, 9216),
          "bsp::crawford_item4_kernel<true, 1, true>": (118, 9216),
          "bsp::crawford_item4_kernel<false, 4, true>": (122, 36864)}


def _kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_notes
    return codeobj_notes.kernels(os.path.join(ROOT, "bspatom_amd", "libbspatom.so"))


def test_resources_of_the_spread_instances():
    inst = {n: v for n, v in _kernels().items() if "crawford_item4_spread_kernel<" in n}
    assert sorted(inst) == ["bsp::crawford_item4_spread_kernel<%s, %d>" % (od, s) for od in ("false", "true") for s in (2, 4)], sorted(inst)
    for name, v in inst.items():
        print(name, v)
        spread = int(name.rstrip(">").split(",")[1])
        assert not v["private_segment_fixed_size"] and not v["vgpr_spill_count"] and not v["sgpr_spill_count"], (name, v)
        assert v["vgpr_count"] + (v["agpr_count"] or 0) <= 128, (name, v)
        assert v["max_flat_workgroup_size"] == 64 * spread, (name, v)
        # Q of four items (4 x 16 x 18 doubles) and phase B's operands of four items (4 x 2 KB), apart
        assert v["group_segment_fixed_size"] == 4 * 16 * 18 * 8 + 4 * 2048, (name, v)


def test_one_wave_instances_are_as_before():
    ks = _kernels()
    for name, (vgpr, lds) in BEFORE.items():
        v = ks[name]
        assert v["vgpr_count"] == vgpr and not v["agpr_count"] and v["group_segment_fixed_size"] == lds, (name, v)
        assert not v["private_segment_fixed_size"] and not v["vgpr_spill_count"] and not v["sgpr_spill_count"], (name, v)
