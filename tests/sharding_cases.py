"""The cases of tests/test_gpu_sharding_sizes.py: the sharded row-band step (regularizepsf_amd/sharding.py) at every patch size and seam form.

A case is (patch size, frame shape, world, HDR seed, lattice).  Frame, K, float64 oracle, local scale and float32 yardstick come from
tests.helpers.LocalCase, one per (case, pad mode).  The table is chosen so that, for both seams and all five kernel pad modes,
`make_band_plans` accepts it, every band owns rows, 10 % of the pixels are dim and at least 25 % of the rows a band receives are dim
(tests/test_sharding_cases.py proves all of it on the CPU), and so that the widths run through every residue modulo 4 at every kernel
generation: the seam rows of a band then start anywhere in their allocation.

``LocalSeam`` stands in for ``_native.Comm`` inside one process: the spill rows travel through a host mailbox, the add is K4.  It waits for
the whole device at every exchange, so what these cases can show is a wrong row, a wrong buffer, a stale buffer and a wrong add - not a race
between two streams that nothing orders.
"""

from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass

import numpy as np

from oracle import regpsf_oracle as orc
from regularizepsf_amd.sharding import make_band_plans, pad_rows
from tests.helpers import DIM, LocalCase, random_transfer

SEAMS = ("exchange", "recompute")
#: the four forms of ShardedApply: name -> (seam, overlap)
FORMS = {"overlap": ("exchange", True), "sequence": ("exchange", False), "pipeline": ("exchange", "pipeline"), "recompute": ("recompute", True)}
#: least share of dim pixels among the rows a band receives.  The HDR frame is constant in amplitude on blocks of 2 N columns, so the share
#: moves in steps of a block: a quarter of the row, less the partial block at the frame's right edge (128 of 518 columns = 0.247 at
#: 400 x 518 / 128, 256 of 1028 = 0.249 at 800 x 1028 / 256 under 'wrap').  At N <= 64 every case has 0.43 or more.
SEAM_ROWS_DIM = 0.24
SEAM_ROWS_DIM_SMALL = 0.43


@dataclass(frozen=True)
class ShardCase:
    n: int
    shape: tuple
    world: int
    seed: int
    lattice: str = "covering"  # "covering"; "rows8": corners every 8 rows and 16 columns; "hole": the covering without one patch
    once: bool = True          # some band runs its seam patches once (two plans, K4 adds their upper rows)
    single: bool = False       # some band that sends is a single lattice row (no other patches: the spill-buffer branch)

    @property
    def name(self):
        tag = "" if self.lattice == "covering" else "-" + self.lattice
        return f"N{self.n}-{self.shape[0]}x{self.shape[1]}-w{self.world}{tag}"

    @property
    def ordered(self):
        """Whether every plan of the case adds a pixel's contributions in a fixed order.  Corners every 8 rows under 32-pixel patches are
        no half-overlap lattice: those plans add with float atomics, in the order the hardware serves them."""
        return self.lattice != "rows8"


CASES = [
    ShardCase(16, (50, 37), 3, 34),
    ShardCase(16, (41, 37), 4, 34, single=True),
    ShardCase(32, (100, 70), 3, 34),
    ShardCase(32, (89, 66), 4, 34, single=True),
    ShardCase(64, (200, 130), 3, 74),
    ShardCase(64, (173, 129), 4, 74, single=True),
    ShardCase(128, (400, 518), 3, 132),
    ShardCase(128, (341, 258), 4, 158, single=True),
    ShardCase(256, (1040, 601), 3, 259),
    ShardCase(256, (800, 1028), 2, 259),
    # a width that is a multiple of 32: the persistent + fused launch (constant, symmetric, wrap) and the fused one (reflect, edge) in bands
    ShardCase(128, (400, 512), 3, 133),
    # a width that is a multiple of 4 at a sweep size (the rows above are 1 or 2 modulo 4 there): seam rows that keep their 16-byte alignment
    ShardCase(16, (50, 36), 3, 34),
    # corners every 8 rows: the patches that reach below a band's line span three lattice rows
    ShardCase(32, (100, 70), 3, 34, lattice="rows8"),
    # a covering without one patch (of a band's last lattice row): no complete lattice, so the colour planes take over from the sweep kernel
    ShardCase(32, (100, 70), 3, 34, lattice="hole"),
]
#: one case per kernel generation for the frame-by-frame test: sweep (16, 64), colour planes of the first generation (the hole), second (128, 256)
FRAME_CASES = [c for c in CASES if (c.n, c.shape, c.lattice) in {(16, (41, 37), "covering"), (64, (173, 129), "covering"), (32, (100, 70), "hole"),
                                                                   (128, (341, 258), "covering"), (256, (1040, 601), "covering")}]
#: (patch size, shape, world, seam) that leave band 0 nothing but the covering's first lattice row, at -N/2: it would own no output row.
#: Both shapes have six lattice rows.  The exchange seam cuts by patch count and isolates the first row at world 6 and world 4; the
#: recompute seam balances own + recomputed patches and comes to it only when every band is a single row (129 x 150 at world 4: served).
NO_ROWS = [(16, (36, 40), 6, "exchange"), (16, (36, 40), 6, "recompute"), (64, (129, 150), 4, "exchange"), (64, (129, 150), 6, "recompute")]
SERVED = [(64, (129, 150), 4, "recompute"), (64, (129, 150), 3, "exchange"), (16, (36, 40), 5, "recompute")]


@functools.lru_cache(maxsize=2)
def transfer(case):
    """(corner list, random complex64 K) of the case's lattice; read-only."""
    coords, k = _transfer(case)
    k.setflags(write=False)
    return coords, k


def _transfer(case):
    h, w = case.shape
    if case.lattice == "rows8":
        assert case.n == 32
        coords = [(r, c) for r in range(-16, h, 8) for c in range(-16, w, 16)]
        rng = np.random.default_rng(case.seed + 1000)
        k = (rng.standard_normal((len(coords), 32, 32)) + 1j * rng.standard_normal((len(coords), 32, 32))).astype(np.complex64)
        return coords, k
    coords, k = random_transfer(case.shape, case.n, case.seed + 1000)
    if case.lattice == "hole":
        plans = make_band_plans(coords, case.n, h, case.world)
        last_row = max(coords[i][0] for i in plans[0].patch_index)
        row = [i for i in plans[0].patch_index if coords[i][0] == last_row]
        drop = row[len(row) // 2]  # a patch in the middle of band 0's last lattice row: one of its seam patches
        keep = [i for i in range(len(coords)) if i != drop]
        return [coords[i] for i in keep], np.ascontiguousarray(k[keep])
    return coords, k


@functools.lru_cache(maxsize=4)
def local_case(case, mode):
    """LocalCase of (case, pad mode): computed once, shared, left unchanged."""
    coords, k = transfer(case)
    lc = LocalCase(case.shape, case.n, case.seed, mode, coords=coords, k=k)
    for a in (lc.image, lc.ref, lc.scale):
        a.setflags(write=False)
    return lc


def band_plans(case, mode, seam):
    return make_band_plans(transfer(case)[0], case.n, case.shape[0], case.world, mode, seam)


def seam_patches(case, band):
    """(seam patches, the other patches) of a band, as ShardedApply(overlap=True) divides them: the patches that reach below the band's own rows."""
    coords = transfer(case)[0]
    own_end = band.out_row0 + band.own_rows
    seam = [i for i in band.patch_index if coords[i][0] + case.n > own_end]
    return seam, [i for i in band.patch_index if i not in set(seam)]


def expected_branches(case, mode, form):
    """{(rank, seam_once, pipeline, overlap)} that ShardedApply's constructor must arrive at, restated from the band plans."""
    seam, overlap = FORMS[form]
    out = set()
    coords = transfer(case)[0]
    for b in band_plans(case, mode, seam):
        linked = seam == "exchange" and case.world > 1 and b.send_rows + b.recv_rows > 0
        once = False
        if linked and overlap is True and b.send_rows > 0:
            seam_index, rest = seam_patches(case, b)
            once = bool(rest) and min(coords[i][0] for i in seam_index) >= b.out_row0
        out.add((b.rank, once, linked and overlap == "pipeline", linked and overlap is True))
    return out


def seam_rows_dim_share(case, mode):
    """Smallest share, over the bands that receive, of dim pixels (local scale <= DIM x the frame's largest) among the rows received."""
    scale = local_case(case, mode).scale
    shares = []
    for b in band_plans(case, mode, "exchange"):
        if b.recv_rows:
            rows = scale[b.out_row0 : b.out_row0 + b.recv_rows]
            shares.append(float(np.count_nonzero(rows <= DIM * scale.max()) / rows.size))
    return min(shares)


def patch_terms(case, mode):
    """Every patch's float64 result after the second window, and its corner in the 2 N-padded frame: the terms of the oracle's overlap-add
    (the steps of tests.helpers.per_patch_reference, which is held against the pinned oracle at 1e-12)."""
    import scipy.fft

    lc = local_case(case, mode)
    n = case.n
    padded = np.pad(lc.image.astype(np.float64), 2 * n, mode=mode)
    window = orc.apodization_window(n, n).astype(np.float64)
    rows = np.array([c[0] for c in lc.coords]) + 2 * n
    cols = np.array([c[1] for c in lc.coords]) + 2 * n
    patches = np.stack([padded[r : r + n, c : c + n] for r, c in zip(rows, cols)])
    return np.real(scipy.fft.ifft2(scipy.fft.fft2(window * patches) * lc.k.astype(np.complex128))) * window, rows, cols


def band_buffer(case, band, terms):
    """What a rank's output buffer holds after its local apply, in float64: its own patches only, rows [out_row0, out_row0 + out_rows)."""
    patches, rows, cols = terms
    n = case.n
    h, w = case.shape
    canvas = np.zeros((h + 4 * n, w + 4 * n))
    for i in band.patch_index:
        canvas[rows[i] : rows[i] + n, cols[i] : cols[i] + n] += patches[i]
    return canvas[2 * n + band.out_row0 : 2 * n + band.out_row0 + band.out_rows, 2 * n : 2 * n + w].copy()


def resident_window_holds(case, band, mode):
    """Every image row that the band's patches read under the pad mode lies inside its resident window."""
    coords = transfer(case)[0]
    rows = np.unique(np.concatenate([np.arange(coords[i][0], coords[i][0] + case.n) for i in band.patch_index]))
    mapped = pad_rows(rows, case.shape[0], mode)
    mapped = mapped[mapped >= 0]
    return bool(mapped.size == 0 or (mapped.min() >= band.image_row0 and mapped.max() < band.image_row0 + band.image_rows))


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------------
class LocalSeam:
    """In-process stand-in for ``_native.Comm`` (the members ``ShardedApply.step`` uses).  The rows sent go to ``mailbox[rank]`` on the host,
    the rows received come from ``mailbox[rank - 1]``; ranks step in the order 0 ... world - 1 and nothing flows upwards, so the entry is
    always there (it is taken out: a rank that reads twice, or before its neighbour wrote, fails).  The add is K4 on the device."""

    stream = None

    def __init__(self, rank, world, mailbox, device=0):
        self.rank, self.world, self.mailbox, self.device = rank, world, mailbox, device

    def seam_exchange(self, send_ptr, send_count, recv_ptr, recv_count, stream=None):
        from regularizepsf_amd import _native

        lib = _native.lib()
        _native.check(lib.rpsf_device_synchronize(self.device))
        if self.rank + 1 < self.world and send_count:
            rows = np.empty(send_count, np.float32)
            _native.check(lib.rpsf_memcpy_d2h(self.device, rows.ctypes.data_as(ctypes.c_void_p), send_ptr, rows.nbytes))
            self.mailbox[self.rank] = rows
        if self.rank > 0 and recv_count:
            rows = self.mailbox.pop(self.rank - 1)
            assert rows.size == recv_count, (rows.size, recv_count)
            _native.check(lib.rpsf_memcpy_h2d(self.device, recv_ptr, rows.ctypes.data_as(ctypes.c_void_p), rows.nbytes))

    def seam_exchange_add(self, send_ptr, send_count, recv_ptr, recv_count, accum_ptr, stream=None):
        from regularizepsf_amd import _native

        self.seam_exchange(send_ptr, send_count, recv_ptr, recv_count, stream)
        if self.rank > 0 and recv_count:
            _native.add_rows(accum_ptr, recv_ptr, recv_count, self.device, stream)


def _release(sh):
    """Give back what a ShardedApply holds now, not when the collector gets to it: hundreds of them pass through one process."""
    sh.synchronize()
    for plan in (sh.plan, sh.seam_plan):
        if plan is not None:
            plan.close()
    if getattr(sh, "_xstream", None) is not None:
        sh._xstream.close()
    for name in ("seam_read", "ev_applied", "ev_exchanged"):
        for event in getattr(sh, name, None) or ():
            event.close()
    buffers = [sh.d_img, sh.d_recv, sh.d_out, getattr(sh, "d_spill", None), *(getattr(sh, "d_seam", None) or ()), *(getattr(sh, "d_outs", None) or ())]
    for buf in buffers:
        if buf is not None:
            buf.free()


def run_sharded(case, mode, form, frames, device=0):
    """The frames one after the other through ``world`` ShardedApply objects of the form, all on one device.  Returns (one stitched float32
    image per frame, {(rank, seam_once, pipeline, overlap)} as the objects report it)."""
    from regularizepsf_amd.sharding import ShardedApply

    seam, overlap = FORMS[form]
    coords, k = transfer(case)
    h, w = case.shape
    mailbox = {}
    ranks = []
    try:
        for rank in range(case.world):
            comm = LocalSeam(rank, case.world, mailbox, device) if seam == "exchange" else None
            ranks.append(ShardedApply(coords, lambda index: k[index], case.n, h, w, rank, case.world, device, comm, pad_mode=mode, seam=seam,
                                      overlap=overlap))
        branches = {(sh.rank, sh.seam_once, sh.pipeline, sh.overlap) for sh in ranks}
        outs = []
        for frame in frames:
            frame = np.ascontiguousarray(frame, np.float32)
            for sh in ranks:
                sh.synchronize()
                sh.upload_rows(frame[sh.band.image_row0 : sh.band.image_row0 + sh.band.image_rows])
            for sh in ranks:
                sh.step()
            assert not mailbox, sorted(mailbox)  # every row sent was received
            full = np.full((h, w), np.nan, np.float32)
            for sh in ranks:
                full[sh.band.out_row0 : sh.band.out_row0 + sh.band.own_rows] = sh.owned_rows()
            outs.append(full)
        return outs, branches
    finally:
        for sh in ranks:
            try:
                _release(sh)
            except Exception:  # noqa: BLE001 - a failure above is the one to report
                pass
