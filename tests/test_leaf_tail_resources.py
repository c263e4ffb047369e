"""Static guard (no GPU) on the list-driven later stage of a bound-pruned tile-format layer (option leaf_tail): k0b_remaining_list (csrc/xrl_k0.hip),
the looped top-k k2_topk_list<NS> (xrl_k2.hip) and the fixed-grid K1 k1_list_kernel<G, NS, 0, LK> (xrl_k1.hip) keep everything in registers, the
looped top-k instantiations sit in the occupancy step of the k2_topk_wave<NS> they stand in for (NS = 16 would not: it is not compiled,
those rows keep the batch-sized grid), and K1's stay within the 128 VGPRs of their four wavefronts per SIMD.  The table it prints is the one in
profiles/leaf_tail.md."""
import re

from test_kernel_resources import demangle, kernel_notes


def waves_per_simd(vgpr):
    return min(8, 512 // (-(-vgpr // 8) * 8))       # gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8


def test_list_kernels_keep_their_registers(tmp_path):
    notes = kernel_notes(tmp_path)
    nice = demangle(sorted(notes))
    by = {re.sub(r"\(.*", "", nice[k]).replace("void ", "").replace("xrl::", "").replace("(anonymous namespace)::", ""): v for k, v in notes.items()}
    k0b = {k: v for k, v in by.items() if k.startswith("k0b_remaining_list")}
    k2l = {k: v for k, v in by.items() if k.startswith("k2_topk_list<")}
    k1l = {k: v for k, v in by.items() if k.startswith("k1_list_kernel<")}
    print("\n| kernel | VGPR | SGPR | scratch | wavefronts per SIMD |\n|---|---|---|---|---|")
    for k, v in sorted({**k0b, **k2l, **k1l}.items()) + sorted((k, v) for k, v in by.items() if k.startswith("k2_topk_wave<")):
        print(f"| `{k}` | {v['vgpr']} | {v['sgpr']} | {v['scratch']} | {waves_per_simd(v['vgpr'])} |")
    assert len(k0b) == 1 and sorted(k2l) == sorted(f"k2_topk_list<{n}>" for n in (1, 2, 4, 8, 13, 24, 32)), (sorted(k0b), sorted(k2l))
    # 16 / 32 lanes per item x units per row x the three row lookups, post-processor class 0
    assert len(k1l) == 18 and all(re.fullmatch(r"k1_list_kernel<(16|32), \d, 0, [012]>", k) for k in k1l), sorted(k1l)
    for k, d in {**k0b, **k2l, **k1l}.items():
        assert d["scratch"] == 0 and d["vgpr_spill"] == 0, (k, d)
    for k, d in k1l.items():
        assert d["vgpr"] <= 128, (k, d)              # amdgpu_waves_per_eu(4, 8)
    for k, d in k2l.items():
        plain = by[k.replace("k2_topk_list", "k2_topk_wave")]
        assert waves_per_simd(d["vgpr"]) == waves_per_simd(plain["vgpr"]), (k, d, plain)
