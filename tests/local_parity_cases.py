"""The cases of tests/test_gpu_local_parity.py and the launch form each of them is labelled with.

Which launch an N = 128 / 256 apply takes is decided by the geometry (regularizepsf_amd/csrc/rpsf_lattice.hpp), and nothing in a result
shows it (the forms are bit-identical), so the shapes below are chosen by those predicates and every figure is labelled with launch():
  * fused_geometry() (plane sum inside the patch launch, per-tile epoch counters): width % 32 == 0 (and 16-byte aligned buffers,
    lattice origin at a multiple of 32 columns: true of every covering here);
  * hot_geometry() (persistent patch workgroups with their per-XCD slot queues, entered only inside a fused launch): pad mode constant,
    symmetric or wrap, width % 4 == 0.
Every other geometry runs one patch per workgroup plus the separate plane-sum kernel.  tests/test_lattice_host.py holds launch() against
the C++ predicates themselves, case by case, without a GPU.
"""

# (N, shape, HDR seed): a lattice a few patches wide with a width that is no multiple of 4, and one tens of patches wide with 16-byte rows
SWEEP_CASES = [(16, (100, 135), 16), (16, (200, 400), 16), (32, (130, 203), 32), (32, (300, 500), 32), (64, (333, 390), 64), (64, (640, 1000), 64)]
# (N, shape, HDR seed): widths 768 / 1024 = fused in every pad mode and persistent in three of them; 651 / 771 = rim patches, an odd
# width, the separate sum kernel
SECOND_CASES = [(128, (640, 768), 128), (128, (520, 651), 129), (256, (768, 1024), 258), (256, (520, 771), 272)]
# one patch size per kernel generation for the batch, streamed, banded and class-API routes: 'symmetric' at widths 640 / 768 is the
# persistent + fused launch (single frames and the fused batch form); 650 with 'reflect' keeps the unfused launch covered beside it
ROUTE_CASES = [(32, (300, 500), 32, "reflect"), (128, (520, 640), 129, "symmetric"), (256, (520, 768), 272, "symmetric"),
               (128, (520, 650), 129, "reflect")]
# all 'symmetric' (the class API's default).  640 / 128 and 768 / 256: every step of the sequence is persistent + fused except the other
# shape (width - 5: unfused), so tile counters, epochs and slot queues live through a bright frame, a shape change and a NaN frame;
# 770 / 256 keeps the unfused launch in the same sequence
ISOLATION_CASES = [(32, (300, 500), 32), (64, (333, 390), 64), (128, (520, 640), 129), (256, (520, 768), 272), (256, (520, 770), 272)]


def launch(n, shape, mode, persist=True, fuse=True):
    """The launch form the library chooses for a whole frame of this shape on a default N = 128 / 256 plan (predicates above)."""
    if n < 128:
        return "sweep"
    fused = fuse and shape[1] % 32 == 0
    if fused and persist and mode in ("constant", "symmetric", "wrap") and shape[1] % 4 == 0:
        return "persistent + fused"
    return "fused, one patch per workgroup" if fused else "separate plane sum"
