"""Static guard on K8's compiled kernels (no GPU): the five metrics_kernel<NS> instantiations and metrics_reduce_kernel exist, use no
scratch and spill nothing, and keep the wavefront-private LDS at 8 KB per wavefront at most.  Prints the table profiles/metrics_device.md
carries (pytest -s)."""
import re

from test_kernel_resources import demangle, kernel_notes

METRICS_WAVES = 4                # wavefronts per workgroup (kMetricsWaves)


def occupancy(vgpr):
    """wavefronts per SIMD the unified 512-register file admits (allocation granule 8), at most 8"""
    return min(8, 512 // max(8, -(-vgpr // 8) * 8))


def test_k8_resources(tmp_path):
    notes = kernel_notes(tmp_path)
    nice = demangle(sorted(notes))
    k8 = {nice[k]: v for k, v in notes.items() if "metrics_kernel<" in nice[k]}
    red = {nice[k]: v for k, v in notes.items() if "metrics_reduce_kernel" in nice[k]}
    print("\nkernel                      VGPR  SGPR  LDS/workgroup  scratch  spills  wavefronts/SIMD")
    seen = set()
    for name, d in sorted(k8.items(), key=lambda kv: int(re.search(r"<(\d+)>", kv[0]).group(1))):
        ns = int(re.search(r"metrics_kernel<(\d+)>", name).group(1))
        seen.add(ns)
        print(f"metrics_kernel<{ns:2d}>          {d['vgpr']:5d} {d['sgpr']:5d} {d['lds']:14d} {d['scratch']:8d} {d['vgpr_spill'] + d['sgpr_spill']:7d} {occupancy(d['vgpr']):16d}")
        assert d["scratch"] == 0 and d["vgpr_spill"] == 0 and d["sgpr_spill"] == 0, (name, d)
        assert d["lds"] == ns * 64 * 8 * METRICS_WAVES and d["lds"] <= 8192 * METRICS_WAVES, (name, d)
    assert seen == {1, 2, 4, 8, 16}, sorted(seen)
    assert len(red) == 1, sorted(red)
    d = next(iter(red.values()))
    print(f"metrics_reduce_kernel       {d['vgpr']:5d} {d['sgpr']:5d} {d['lds']:14d} {d['scratch']:8d} {d['vgpr_spill'] + d['sgpr_spill']:7d} {occupancy(d['vgpr']):16d}")
    assert d["scratch"] == 0 and d["vgpr_spill"] == 0 and d["sgpr_spill"] == 0 and d["lds"] == 0, d
