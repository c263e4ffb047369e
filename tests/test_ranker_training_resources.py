"""Static guard on K13's compiled kernels (no GPU): the seven k13_* kernels exist, use no LDS and no scratch memory and spill no vector
register; k13_solve keeps a register count at which four wavefronts share a SIMD -- the slot count (kTrainMaxSlots = 16 per CU x 256)
assumes it.  k13_solve's arguments and fp64 scalars are all uniform, so it is scalar registers that run out: the compiler parks some
in lanes of vector registers (reported as SGPR spills; with scratch == 0 none of them reaches memory).  That count is printed, not
bounded: it moves with the compiler.  Prints the table profiles/ranker_training.md carries (pytest -s)."""
import re

from test_kernel_resources import demangle, kernel_notes
from test_metrics_resources import occupancy


def test_k13_resources(tmp_path):
    notes = kernel_notes(tmp_path)
    nice = demangle(sorted(notes))
    k13 = {nice[k]: v for k, v in notes.items() if "k13_" in nice[k]}
    names = {re.search(r"k13_\w+", n).group(0) for n in k13}
    assert names == {"k13_check", "k13_same", "k13_labels", "k13_sizes", "k13_solve", "k13_label_counts", "k13_place"}, sorted(names)
    print("\nkernel                      VGPR  SGPR  LDS/workgroup  scratch  VGPR spills  SGPRs parked in VGPR lanes  wavefronts/SIMD")
    for name, d in sorted(k13.items()):
        short = re.search(r"k13_\w+", name).group(0)
        print(f"{short:27s} {d['vgpr']:5d} {d['sgpr']:5d} {d['lds']:14d} {d['scratch']:8d} {d['vgpr_spill']:12d} {d['sgpr_spill']:27d} {occupancy(d['vgpr']):16d}")
        assert d["scratch"] == 0 and d["vgpr_spill"] == 0 and d["lds"] == 0, (name, d)
        if short == "k13_solve":
            assert occupancy(d["vgpr"]) >= 4, (name, d)
        else:
            assert d["sgpr_spill"] == 0, (name, d)
