"""Static guard (no GPU) on the fused first stage of the leaf (csrc/xrl_k1t.hip, k1t_kernel<32, NR, PPC, LK, BUF, SEL = true>): every
instantiation keeps everything in registers and stays at the kernel's own floor of five wavefronts per SIMD (amdgpu_waves_per_eu(5, 8):
<= 96 VGPRs), like the plain kernel it replaces -- the selection state takes the accumulators' place after the feature loop."""
from test_kernel_resources import demangle, kernel_notes


def test_fused_leaf_kernels_keep_their_register_budget(tmp_path):
    notes = kernel_notes(tmp_path)
    nice = demangle(sorted(notes))
    by = {nice[k]: v for k, v in notes.items()}
    fused = {k: v for k, v in by.items() if "k1t_kernel<32, " in k and k.split(">")[0].endswith(", true")}
    plain = {k: v for k, v in by.items() if "k1t_kernel<32, " in k and k.split(">")[0].endswith(", false")}
    # NR 1..4 x post-processor class x row lookup x addressing
    assert len(fused) == 32 and len(plain) == 32, (sorted(fused), sorted(plain))
    for k, d in fused.items():
        assert d["scratch"] == 0 and d["vgpr_spill"] == 0 and d["vgpr"] <= 96, (k, d)
    # only 32-lane items are fused
    assert not [k for k in by if "k1t_kernel<" in k and "k1t_kernel<32, " not in k and k.split(">")[0].endswith(", true")]
