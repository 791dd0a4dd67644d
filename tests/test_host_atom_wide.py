"""Host: the wide-tile atom kernels of the built library.  atom_wide_kernel<FFN, MODE, RT> (scann_kernels.hip) runs 96-row tiles at two
workgroups per CU: its register budget is the whole file of a two-wave SIMD slot (256 VGPRs).  Read from the BUILT library's kernel
descriptors, as tests/test_host.py reads atom_kernel's.  And the launch code's height rule, as the source lines that state it."""
import os
import re

import abi_checks


WIDE = re.compile(r"_ZN5scann16atom_wide_kernelILb(\d)ELi(\d)ELi(\d)EEEv")


def test_wide_atom_kernels_use_no_scratch(hip_lib):
    """Every atom_wide_kernel instantiation: 0 bytes of scratch, at most 256 VGPRs; and the two that launch_atom launches exist --
    FFN = true, MODE 0 (layers 1 .. L-1) and MODE 2 (after_Lc, gq, gk), RT = 3 (128 rows won at no launch size and is not shipped)"""
    from scann import _hip

    kern = abi_checks.device_kernels(_hip.LIB_PATH)
    seen = set()
    for name, (scratch, vgpr) in kern.items():
        if "atom_wide_kernel" not in name:
            continue
        m = WIDE.match(name)
        assert m, name
        seen.add(tuple(int(g) for g in m.groups()))
        print(name, scratch, vgpr)
        assert scratch == 0, (name, scratch, vgpr)
        assert vgpr <= 256, (name, vgpr)
    assert seen == {(1, 0, 3), (1, 2, 3)}, sorted(seen)


def test_height_rule_of_the_plain_inference_launches():
    """launch_atom's automatic choice for the launches that have the wide kernel: 32 rows up to three tiles per CU, 64 and then 96 rows
    up to two per CU, 64 beyond; everything else keeps the 32,768-atom switch tests/size_batches.py restates"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scann--material_amd", "csrc", "scann_kernels.hip")) as f:
        src = f.read()
    rule = ("  if (!wide || n_cu <= 0) return rows;\n", "  if ((a.n_atom + 31) / 32 <= 3 * n_cu) return 32;\n  if ((a.n_atom + 63) / 64 <= 2 * n_cu) return 64;\n"
            "  if ((a.n_atom + 95) / 96 <= 2 * n_cu) return 96;\n  return 64;\n")
    assert all(r in src for r in rule)
    assert src.index("const int rows = a.n_atom <= 32 * 1024 ? 32 : 64;") < src.index(rule[0]) < src.index(rule[1])
