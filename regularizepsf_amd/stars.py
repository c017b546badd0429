"""Star positions for ``ArrayPSFBuilder.build(..., stars=...)`` on the GPU.

``find_stars`` is this package's own detector, modelled on what ``sep.Background`` plus ``sep.extract`` do without deblending:
a sigma-clipped background mesh, a bilinear surface through it, a 3 x 3 smoothing filter, a threshold in units of the global
background rms, 8-connected components and their flux-weighted centroids (the definition is DESIGN.md 3.7).

It is NOT ``sep``: deblending is an option (``deblend=True``, off by default) and then one watershed level on the filtered residual
with a significance test per basin, not ``sep``'s multi-threshold tree; without it touching stars come out as
one detection at their common centroid.  The box statistic is a clipped median / mean rule without ``sep``'s histogram mode estimate,
and the background surface is bilinear where ``sep``'s is bicubic.  Positions differ from ``sep``'s for blended or extended sources.
Isolated stars on a smooth background - what a PSF model is built from - come out at their centroids.

Four kernel groups behind ``rpsf_stars_*`` (include/rpsf.h) do the work on whole frames: the mesh (S1), detection (S2),
labelling (S3) and moments (S4); with ``deblend=True`` a fifth (D1 - D4) splits blended components after S4.  For host frames the host keeps the bookkeeping: filling and median-filtering the mesh (a few
thousand numbers, ``filter_mesh``) between S1 and S2.  Device frames (``DeviceArray`` or anything with
``__cuda_array_interface__``) take the fused route of DESIGN.md 3.11, which ``ArrayPSFBuilder(..., finder="device")`` takes for
every frame: the frame is read where it lies, kernel S1b does ``filter_mesh``'s work on the device - the same bits - and nothing but
the positions comes back.

``star_catalog`` is ``find_stars`` with a catalogue per frame instead of bare positions: one more kernel (S5, ``rpsf_stars_measure``)
walks every detection again around its finished centroid and returns central second moments, the peak and the bounding box; the
ellipse (``a``, ``b``, ``theta``, ``elongation``) is derived from them here in NumPy float64.  The moments are NOT ``sep``'s either: no
1 / 12 pixel term, no clamp of a singular matrix, and the footprint is this detector's.

``star_photometry`` measures at positions the caller supplies - ``find_stars``' output, a filtered catalogue, any list - instead of at
what this detector finds: circular apertures at several radii with sub-pixel coverage (kernel S6, ``rpsf_stars_photometry``; DESIGN.md
3.7 "Apertures"), on the outermost one the peak and the moments around the given position, and a half-light radius from the curve of
growth.  The footprint is the aperture, not the threshold's, so the same stars can be compared before and after ``apply``.  It is NOT
``sep``'s ``sum_circle`` / ``flux_radius``: a sub-sample counts when ``q <= R^2``, there is no error column and no 1 / 12 term, and
masked pixels are excluded and reported through ``coverage``, not corrected for.

``refine_stars`` moves given positions to their Gaussian-windowed centroids (kernel S7, ``rpsf_stars_refine``; DESIGN.md 3.7 "Windowed
positions"): the iteration ``p <- p + 2 sum w d (r - p) / sum w d`` with ``w = exp(-q / 2 sigma^2)`` inside ``q <= (4 sigma)^2``, and the
windowed second moments at the position it ends at.  The builder's ``finder_options={"refine_sigma": s}`` applies it to the detections of
the fused route.  It is NOT ``sep``'s ``winpos``: no sub-pixel sampling of the window's
rim, the comparison is ``<=``, there is no error column, and masked pixels are excluded and reported through ``coverage``, not corrected
for.

``fit_stars`` judges a PSF model by the stars: every star is fitted, by linear least squares over a disc, with the cell of the model it
belongs to, bilinearly interpolated to the star's position (kernel S8, ``rpsf_stars_fit``; DESIGN.md 3.7 "Model fits"), and the residual
of that fit is reported; ``cell_fit_summary`` folds the stars into one row per cell, the map that shows where a model is bad.  It is
NOT a PSF-photometry package's fit: the weights are uniform - no error column, no variance weighting -, the position is given and
not fitted (``refine_stars`` supplies positions), the interpolation is bilinear and does not conserve flux below the pixel scale, and
masked pixels are excluded and reported through ``coverage``, not corrected for.

``fit_positions`` lets the model say where a star is: a Gauss-Newton iteration of ``(row, col)`` around ``fit_stars``' linear fit, with the
exact gradient of the bilinearly interpolated cell (kernel S9, ``rpsf_stars_fit_positions``; DESIGN.md 3.7 "Fitted positions"), and
``fit_stars``' own row at the position it ends at.  It is the other half of the effective-PSF loop: build a model, fit positions with it,
rebuild at the fitted positions.  It shares ``fit_stars``' limits - uniform weights, no error column, bilinear interpolation, masked
pixels excluded and not corrected for - and adds its own: the cell is fixed at the input position and one star is fitted at a time.

``subtract_stars`` draws the fitted stars with their cells of the model and takes them out of the frame, and ``render_stars`` draws them
on an empty frame (kernel S10, ``rpsf_stars_render``; DESIGN.md 3.7 "Model and residual frames").  The kernel gathers: a workgroup owns a
tile of output pixels and every pixel adds its stars in ascending star index, so the bits do not depend on scheduling.  The model is cut
at the radius ``R``, interpolated bilinearly, and the per-star fitted constant is not subtracted.

``fit_groups`` is ``fit_stars`` for crowded fields: stars whose fit discs overlap are fitted together, one flux each and one shared
constant, positions fixed (kernel S11, ``rpsf_stars_fit_groups``; DESIGN.md 3.7 "Group fits"); ``star_groups`` is the grouping alone, on
the host.  It uses ``fit_stars``' and ``subtract_stars``' definitions, so the three agree bit for bit where they meet, and it shares
their limits: uniform weights, bilinear interpolation, the model cut at ``R``, the cell fixed.  Positions are not fitted jointly, and
nothing guards near-coincident stars but ``DEGENERATE`` at a non-positive pivot.

``fit_stars_weighted`` is ``fit_stars`` with a weight ``1 / v`` per pixel and the formal errors of flux and background (kernel S12,
``rpsf_stars_fit_weighted``; DESIGN.md 3.7 "Weighted fits"): ``v`` from a variance map or from ``sky_variance + max(pixel, 0) / gain``, a pixel
without a usable variance left out like a masked one, ``chi2`` in units of the variances, ``flux_err``, ``snr`` and ``chi2_reduced`` per star.
With ``v = 1`` it is ``fit_stars`` bit for bit.  Positions are fixed, the model is bilinear and cut at ``R``, the errors are what the given
variances imply and nothing else, and ``fit_positions`` and ``fit_groups`` stay unweighted.
"""

from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from regularizepsf_amd.builder import _device_frames, _frames, star_positions
from regularizepsf_amd.device_array import is_device_array
from regularizepsf_amd.exceptions import IncorrectShapeError

MIN_BOX, MAX_BOX = 8, 128
# a shape row of kernel S5 (RPSF_STARS_SHAPE_COLUMNS float64, include/rpsf.h), and the catalogue: those columns and the derived ones
SHAPE_COLUMNS = ("row", "col", "flux", "area", "peak", "peak_row", "peak_col", "row_min", "row_max", "col_min", "col_max", "abs_flux",
                 "rr", "cc", "rc")
CATALOG_FIELDS = (*SHAPE_COLUMNS, "a", "b", "theta", "elongation")
CATALOG_DTYPE = np.dtype([(name, np.float64) for name in CATALOG_FIELDS])
# a photometry row of kernel S6 for m radii (RPSF_STARS_PHOTOMETRY_COLUMNS(m) float64): row, col, flux[m], N_use[m], N_all[m], then these
PHOTOMETRY_SUMS = ("abs_flux", "mr", "mc", "mrr", "mcc", "mrc", "peak", "peak_row", "peak_col")
MAX_RADII, MAX_RADIUS, MAX_SUBPIX, MAX_COORD = 8, 64.0, 8, 2.0 ** 20
# a row of kernel S7 (RPSF_STARS_REFINE_COLUMNS float64) and its flags
REFINE_COLUMNS = ("row0", "col0", "row", "col", "sigma", "niter", "flags", "step_row", "step_col", "n_use", "n_all", "flux", "abs_flux", "mr",
                  "mc", "mrr", "mcc", "mrc")
NO_FLUX, RAN_AWAY, NOT_CONVERGED = 1, 2, 4
MIN_SIGMA, MAX_SIGMA, MAX_ITER = 0.5, 16.0, 64
# a row of kernel S8 (RPSF_STARS_FIT_COLUMNS float64) and its flags
FIT_COLUMNS = ("row", "col", "cell", "flags", "n_use", "n_all", "sm", "sm_all", "smm", "sd", "sdm", "sdd", "flux", "background", "chi2", "abs_res",
               "peak_res", "peak_e", "peak_row", "peak_col")
NO_MESH, TOO_FEW, DEGENERATE, BAD_CELL = 1, 2, 4, 8
MIN_MODEL, MAX_MODEL = 4, 256
# an iteration row of kernel S9 (RPSF_STARS_FITPOS_COLUMNS float64) and its flags
FITPOS_COLUMNS = ("row0", "col0", "row", "col", "niter", "flags", "step_row", "step_col")
FITPOS_RAN_AWAY, FITPOS_NOT_CONVERGED, FITPOS_SINGULAR, FITPOS_SKIPPED = 1, 2, 4, 8
# a row of kernel S11 (RPSF_STARS_FIT_GROUPS_COLUMNS float64): S8's columns, then the group's; the flag of rpsf_stars_link_groups
GROUP_COLUMNS = (*FIT_COLUMNS, "group", "group_size", "group_n", "group_chi2", "group_abs_res")
CROWDED, MAX_GROUP = 16, 8
# a row of kernel S12 (RPSF_STARS_FIT_WEIGHTED_COLUMNS float64; S8's flags) and its variance modes (RPSF_STARS_VARIANCE_*)
FITW_COLUMNS = ("row", "col", "cell", "flags", "n_use", "n_all", "sm", "sm_all", "sw", "swm", "swmm", "swd", "swdm", "swdd", "flux", "background",
                "var_flux", "var_background", "cov", "chi2", "abs_res", "peak_res", "peak_e", "peak_row", "peak_col")
VARIANCE_MAP, VARIANCE_MODEL = 0, 1
# the modes of kernel S10 (RPSF_STARS_RENDER_* of include/rpsf.h)
RENDER_MODEL, RENDER_RESIDUAL, RENDER_RESIDUAL_MESH = 0, 1, 2
DEBLEND_OPTIONS = {"deblend": False, "deblend_contrast": 0.005, "deblend_prominence": 1.0}  # contrast: sep's deblend_cont


def deblend_options(deblend, deblend_contrast, deblend_prominence) -> tuple[bool, float, float]:
    """The three deblend options of ``find_stars`` and ``finder_options``, range-checked."""
    if not isinstance(deblend, (bool, np.bool_)):
        msg = f"deblend must be True or False, not {deblend!r}"
        raise ValueError(msg)
    contrast, prominence = float(deblend_contrast), float(deblend_prominence)
    if not 0.0 <= contrast <= 1.0:
        msg = f"deblend_contrast must lie in 0 ... 1, got {deblend_contrast}"
        raise ValueError(msg)
    if not (prominence >= 0.0 and np.isfinite(prominence)):
        msg = f"deblend_prominence must be finite and not negative, got {deblend_prominence}"
        raise ValueError(msg)
    return bool(deblend), contrast, prominence


class _Finder:
    """A native finder handle: one frame shape, one background box."""

    def __init__(self, shape: tuple[int, int], box: int, device: int = 0) -> None:
        from regularizepsf_amd import _native

        self._native, self.shape, self.box, self.device = _native, (int(shape[0]), int(shape[1])), int(box), int(device)
        self.mesh_shape = (-(-self.shape[0] // self.box), -(-self.shape[1] // self.box))
        self._handle = ctypes.c_void_p()
        _native.check(_native.lib().rpsf_stars_create(ctypes.byref(self._handle), device, self.shape[0], self.shape[1], self.box))

    def background(self, frame: np.ndarray, mask: np.ndarray | None) -> tuple[np.ndarray, np.ndarray]:
        """Upload the frame and the mask; the raw mesh (level, rms), NaN where a box has no usable pixel."""
        n = self._native
        if frame.dtype != np.float32:
            frame = frame.astype(np.float64, copy=False)
        frame = np.ascontiguousarray(frame)
        flags = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        level, rms = np.empty(self.mesh_shape), np.empty(self.mesh_shape)
        n.check(n.lib().rpsf_stars_background(self._handle, n._ptr(frame), int(frame.dtype == np.float64),
                                              None if flags is None else n._ptr(flags), n._ptr(level), n._ptr(rms)))
        return level, rms

    def detect(self, level: np.ndarray, threshold_abs: float, min_area: int, max_area: int | None) -> np.ndarray:
        """Detections of the frame uploaded last: (k, 4) rows of (row, col, flux, area)."""
        n = self._native
        level = np.ascontiguousarray(level, np.float64)
        count = ctypes.c_size_t(0)
        n.check(n.lib().rpsf_stars_detect(self._handle, n._ptr(level), float(threshold_abs), int(min_area),
                                          -1 if max_area is None else int(max_area), ctypes.byref(count)))
        out = np.empty((count.value, 4))
        n.check(n.lib().rpsf_stars_positions(self._handle, 0, count.value, n._ptr(out)))
        return out

    def background_device(self, frame, mask: np.ndarray | None) -> None:
        """The fused route's S1 and S1b: ``frame`` is a host array (uploaded once) or a 2-D ``DeviceArray`` (read where it lies); the
        meshes stay on the device."""
        n = self._native
        flags = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        flags_ptr = None if flags is None else n._ptr(flags)
        if isinstance(frame, np.ndarray):
            if frame.dtype != np.float32:
                frame = frame.astype(np.float64, copy=False)
            frame = np.ascontiguousarray(frame)
            n.check(n.lib().rpsf_stars_background_host(self._handle, n._ptr(frame), int(frame.dtype == np.float64), flags_ptr))
        else:
            frame.synchronize()  # the finder's launches are on the null stream
            view = frame._view2d()
            n.check(n.lib().rpsf_stars_background_view(self._handle, ctypes.byref(view), flags_ptr))

    def background_scaled(self, frame: np.ndarray, scale: int, mask: np.ndarray | None) -> None:
        """The same for a finder of the scaled shape: the unscaled host frame is uploaded once and upscaled on the device."""
        n = self._native
        if frame.dtype != np.float32:
            frame = frame.astype(np.float64, copy=False)
        frame = np.ascontiguousarray(frame)
        flags = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        n.check(n.lib().rpsf_stars_background_scaled(self._handle, n._ptr(frame), int(frame.dtype == np.float64), frame.shape[0],
                                                     frame.shape[1], int(scale), None if flags is None else n._ptr(flags)))

    def detect_device(self, threshold: float, min_area: int, max_area: int | None) -> np.ndarray:
        """Detections of the frame given to ``background_device`` / ``background_scaled`` last, the threshold in units of the global
        rms S1b left on the device: (k, 4) rows of (row, col, flux, area)."""
        n = self._native
        count = ctypes.c_size_t(0)
        n.check(n.lib().rpsf_stars_detect_device(self._handle, float(threshold), int(min_area), -1 if max_area is None else int(max_area),
                                                 ctypes.byref(count)))
        out = np.empty((count.value, 4))
        n.check(n.lib().rpsf_stars_positions(self._handle, 0, count.value, n._ptr(out)))
        return out

    def filter_mesh(self, level: np.ndarray, rms: np.ndarray, threshold: float):
        """S1b alone on raw meshes of the finder's mesh shape: (level, rms, global rms, T, none); with ``none`` = 1 (no valid node) only
        T (+inf) means anything."""
        n = self._native
        level, rms = np.ascontiguousarray(level, np.float64), np.ascontiguousarray(rms, np.float64)
        if level.shape != self.mesh_shape or rms.shape != self.mesh_shape:
            msg = f"the meshes must have the finder's mesh shape {self.mesh_shape}"
            raise IncorrectShapeError(msg)
        level_f, rms_f = np.empty(self.mesh_shape), np.empty(self.mesh_shape)
        global_rms, T, none = ctypes.c_double(np.nan), ctypes.c_double(np.nan), ctypes.c_int(-1)
        n.check(n.lib().rpsf_stars_filter_mesh(self._handle, n._ptr(level), n._ptr(rms), float(threshold), n._ptr(level_f), n._ptr(rms_f),
                                               ctypes.byref(global_rms), ctypes.byref(T), ctypes.byref(none)))
        return level_f, rms_f, global_rms.value, T.value, none.value

    def frame_ptr(self) -> int:
        """The finder's float32 frame on the device (valid until the next frame or ``close``)."""
        ptr = ctypes.c_void_p()
        self._native.check(self._native.lib().rpsf_stars_frame(self._handle, ctypes.byref(ptr), None, None))
        return ptr.value

    def set_deblend(self, on: bool, contrast: float = 0.005, prominence: float = 1.0) -> None:
        """Every following ``detect`` / ``detect_device`` splits blended components (D1 - D4), or, ``on`` False, does what it did."""
        self._native.check(self._native.lib().rpsf_stars_set_deblend(self._handle, int(bool(on)), float(contrast), float(prominence)))

    def basins(self, f: np.ndarray, detected: np.ndarray) -> np.ndarray:
        """D1 alone: per detected pixel the linear index of its basin's peak in ``f``, -1 elsewhere."""
        n = self._native
        f, flags = np.ascontiguousarray(f, np.float64), np.ascontiguousarray(detected, np.uint8)
        if f.shape != self.shape or flags.shape != self.shape:
            msg = f"f and the mask must have the finder's shape {self.shape}"
            raise IncorrectShapeError(msg)
        peak = np.empty(self.shape, np.int32)
        n.check(n.lib().rpsf_stars_basins(self._handle, n._ptr(f), n._ptr(flags), n._ptr(peak)))
        return peak

    def measure(self) -> np.ndarray:
        """Kernel S5 on the rows of the last ``detect`` / ``detect_device``: (k, len(SHAPE_COLUMNS)) float64, the first four columns the
        detect's rows bit for bit.  An error when there is no such detect or the frame or mesh has been replaced since."""
        n = self._native
        count = ctypes.c_size_t(0)
        n.check(n.lib().rpsf_stars_measure(self._handle, ctypes.byref(count)))
        out = np.empty((count.value, len(SHAPE_COLUMNS)))
        n.check(n.lib().rpsf_stars_shapes(self._handle, 0, count.value, n._ptr(out)))
        return out

    def shape_ms(self) -> float:
        """Device time of the last S5."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_stars_shape_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def photometry(self, positions: np.ndarray, radii, subpix: int = 5, use_mesh: bool = True) -> np.ndarray:
        """Kernel S6 on the frame given to ``background_device`` / ``background_scaled`` last, at ``positions`` ((k, 2) of (row, col)):
        (k, photometry_columns(m)) float64.  Nothing of the finder is replaced: ``detect`` rows and ``measure`` stay what they were."""
        n = self._native
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        radii = np.ascontiguousarray(radii, np.float64).ravel()
        out = np.empty((len(positions), photometry_columns(len(radii))))
        n.check(n.lib().rpsf_stars_photometry(self._handle, len(positions), n._ptr(positions), len(radii), n._ptr(radii), int(subpix),
                                              int(bool(use_mesh)), n._ptr(out)))
        return out

    def photometry_ms(self) -> float:
        """Device time of the last S6; 0.0 when it launched nothing."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_stars_photometry_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def refine(self, positions: np.ndarray, sigma, max_iter: int = 16, eps: float = 1e-4, max_shift: float = 2.0,
               use_mesh: bool = True) -> np.ndarray:
        """Kernel S7 on the frame given to ``background_device`` / ``background_scaled`` last, from ``positions`` ((k, 2) of (row, col)) with
        the window ``sigma`` (a scalar or one per position): (k, len(REFINE_COLUMNS)) float64.  Nothing of the finder is replaced."""
        n = self._native
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        sigma = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, np.float64), (len(positions),)))
        out = np.empty((len(positions), len(REFINE_COLUMNS)))
        n.check(n.lib().rpsf_stars_refine(self._handle, len(positions), n._ptr(positions), n._ptr(sigma), int(max_iter), float(eps),
                                          float(max_shift), int(bool(use_mesh)), n._ptr(out)))
        return out

    def refine_ms(self) -> float:
        """Device time of the last S7; 0.0 when it launched nothing."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_stars_refine_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def fit(self, model, positions: np.ndarray, cells, radius: float, fit_background: bool = True, use_mesh: bool = True) -> np.ndarray:
        """Kernel S8 on the frame given to ``background_device`` / ``background_scaled`` last: ``model`` (a ``_Model``) fitted at ``positions``
        ((k, 2) of (row, col)), each with its cell of ``cells`` ((k,) integers): (k, len(FIT_COLUMNS)) float64.  Nothing of the finder is
        replaced."""
        n = self._native
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        cells = np.ascontiguousarray(cells, np.int32).ravel()
        if len(cells) != len(positions):
            msg = f"{len(cells)} cells for {len(positions)} positions"
            raise ValueError(msg)
        out = np.empty((len(positions), len(FIT_COLUMNS)))
        n.check(n.lib().rpsf_stars_fit(self._handle, model._handle, len(positions), n._ptr(positions), n._ptr(cells), float(radius),
                                       int(bool(fit_background)), int(bool(use_mesh)), n._ptr(out)))
        return out

    def fit_ms(self) -> float:
        """Device time of the last S8; 0.0 when it launched nothing."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_stars_fit_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def variance(self, frame) -> None:
        """The variance frame of ``fit_weighted``'s map mode: a host array (uploaded, float64 rounded to float32 once) or a 2-D
        ``DeviceArray`` (read where it lies), of the finder's shape.  Nothing else of the finder changes; it stays until the next call."""
        n = self._native
        if isinstance(frame, np.ndarray):
            if frame.shape != self.shape:
                msg = f"A variance frame of shape {frame.shape} does not fit a finder of shape {self.shape}"
                raise IncorrectShapeError(msg)
            if frame.dtype != np.float32:
                frame = frame.astype(np.float64, copy=False)
            frame = np.ascontiguousarray(frame)
            n.check(n.lib().rpsf_stars_variance_host(self._handle, n._ptr(frame), int(frame.dtype == np.float64)))
        else:
            frame.synchronize()  # the finder's launches are on the null stream
            view = frame._view2d()
            n.check(n.lib().rpsf_stars_variance_view(self._handle, ctypes.byref(view)))

    def fit_weighted(self, model, positions: np.ndarray, cells, radius: float, fit_background: bool = True, use_mesh: bool = True,
                     sky_variance: float | None = None, gain: float = np.inf) -> np.ndarray:
        """Kernel S12 on the frame given to ``background_device`` / ``background_scaled`` last, S8's arguments: ``sky_variance`` None takes
        the variance frame given to ``variance`` last, a number the noise model ``sky_variance + max(pixel, 0) / gain``.
        (k, len(FITW_COLUMNS)) float64.  Nothing of the finder is replaced."""
        n = self._native
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        cells = np.ascontiguousarray(cells, np.int32).ravel()
        if len(cells) != len(positions):
            msg = f"{len(cells)} cells for {len(positions)} positions"
            raise ValueError(msg)
        out = np.empty((len(positions), len(FITW_COLUMNS)))
        mode, sky = (VARIANCE_MAP, 0.0) if sky_variance is None else (VARIANCE_MODEL, float(sky_variance))
        n.check(n.lib().rpsf_stars_fit_weighted(self._handle, model._handle, len(positions), n._ptr(positions), n._ptr(cells), float(radius),
                                                int(bool(fit_background)), int(bool(use_mesh)), mode, sky, float(gain), n._ptr(out)))
        return out

    def fit_weighted_ms(self) -> float:
        """Device time of the last S12; 0.0 when it launched nothing."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_stars_fit_weighted_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def fit_positions(self, model, positions: np.ndarray, cells, radius: float, fit_background: bool = True, max_iter: int = 16,
                      eps: float = 1e-4, max_shift: float = 2.0, max_step: float = 0.5, use_mesh: bool = True) -> tuple[np.ndarray, np.ndarray]:
        """Kernel S9 and then S8 on the frame given to ``background_device`` / ``background_scaled`` last: ``positions`` iterated with their
        cells of ``model``, and S8's rows where they end.  ((k, len(FITPOS_COLUMNS)), (k, len(FIT_COLUMNS))) float64.  Nothing of the finder
        is replaced."""
        n = self._native
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        cells = np.ascontiguousarray(cells, np.int32).ravel()
        if len(cells) != len(positions):
            msg = f"{len(cells)} cells for {len(positions)} positions"
            raise ValueError(msg)
        steps, fits = np.empty((len(positions), len(FITPOS_COLUMNS))), np.empty((len(positions), len(FIT_COLUMNS)))
        n.check(n.lib().rpsf_stars_fit_positions(self._handle, model._handle, len(positions), n._ptr(positions), n._ptr(cells), float(radius),
                                                 int(bool(fit_background)), int(max_iter), float(eps), float(max_shift), float(max_step),
                                                 int(bool(use_mesh)), n._ptr(steps), n._ptr(fits)))
        return steps, fits

    def fit_positions_ms(self) -> float:
        """Device time of the last S9 with the S8 behind it; 0.0 when it launched nothing."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_stars_fit_positions_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def fit_groups(self, model, positions: np.ndarray, cells, radius: float, fit_background: bool = True, use_mesh: bool = True,
                   link: float | None = None, max_group: int = MAX_GROUP) -> np.ndarray:
        """Kernel S11, and S8 for every star that is alone, on the frame given to ``background_device`` / ``background_scaled`` last: the
        stars of ``positions`` no further than ``link`` (None: ``2 radius``) from one another fitted together with their cells of
        ``model``: (k, len(GROUP_COLUMNS)) float64.  Nothing of the finder is replaced."""
        n = self._native
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        cells = np.ascontiguousarray(cells, np.int32).ravel()
        if len(cells) != len(positions):
            msg = f"{len(cells)} cells for {len(positions)} positions"
            raise ValueError(msg)
        out = np.empty((len(positions), len(GROUP_COLUMNS)))
        n.check(n.lib().rpsf_stars_fit_groups(self._handle, model._handle, len(positions), n._ptr(positions), n._ptr(cells), float(radius),
                                              int(bool(fit_background)), int(bool(use_mesh)), 2.0 * float(radius) if link is None else float(link),
                                              int(max_group), n._ptr(out)))
        return out

    def fit_groups_ms(self) -> float:
        """Device time of the last S11 with the S8 beside it; 0.0 when it launched nothing."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_stars_fit_groups_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def render(self, model, positions: np.ndarray, flux, cells, radius: float, mode: int = RENDER_RESIDUAL, dtype=np.float32,
               out=None) -> tuple:
        """Kernel S10: the stars at ``positions`` ((k, 2) of (row, col)) drawn with ``flux`` ((k,) float64) and their cells of ``model``.
        ``mode``: ``RENDER_MODEL`` (the sum alone; nothing of the frame is read), ``RENDER_RESIDUAL`` (the frame given to
        ``background_device`` / ``background_scaled`` last, minus the sum) or ``RENDER_RESIDUAL_MESH`` (the frame minus its mesh, minus
        the sum).  ``out``: None for a host array of the finder's shape and ``dtype`` (float32 or float64), or a C-contiguous
        ``DeviceArray`` of that shape and dtype on the finder's device, which the kernel writes and which is returned.  ``(frame, the
        number of stars drawn)``.  Nothing of the finder is replaced."""
        n = self._native
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        flux = np.ascontiguousarray(flux, np.float64).ravel()
        cells = np.ascontiguousarray(cells, np.int32).ravel()
        if len(cells) != len(positions) or len(flux) != len(positions):
            msg = f"{len(flux)} fluxes and {len(cells)} cells for {len(positions)} positions"
            raise ValueError(msg)
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            msg = f"dtype must be float32 or float64, not {dtype}"
            raise TypeError(msg)
        if out is None:
            result = np.empty(self.shape, dtype)
            target, on_device = n._ptr(result), 0
        else:
            _check_render_out(out, self.shape, dtype)
            out.synchronize()  # the finder's launches are on the null stream
            result, target, on_device = out, ctypes.c_void_p(out.ptr), 1
        drawn = ctypes.c_size_t(0)
        n.check(n.lib().rpsf_stars_render(self._handle, model._handle, len(positions), n._ptr(positions), n._ptr(flux), n._ptr(cells),
                                          float(radius), int(mode), int(dtype == np.float64), on_device, target, ctypes.byref(drawn)))
        return result, drawn.value

    def render_ms(self) -> float:
        """Device time of the last S10."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_stars_render_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def deblend_info(self) -> tuple[int, int, int]:
        """Of the last detect: components, basins, split components."""
        counts = [ctypes.c_size_t(0) for _ in range(3)]
        self._native.check(self._native.lib().rpsf_stars_deblend_info(self._handle, *(ctypes.byref(c) for c in counts)))
        return tuple(c.value for c in counts)

    def deblend_ms(self) -> float:
        """Device time of the last D1 - D4."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_stars_deblend_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def mesh_ms(self) -> float:
        """Device time of the last S1b."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_stars_mesh_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def label(self, detected: np.ndarray) -> np.ndarray:
        """S3 alone: per detected pixel the smallest linear index of its 8-connected component, -1 elsewhere."""
        n = self._native
        flags = np.ascontiguousarray(detected, np.uint8)
        labels = np.empty(self.shape, np.int32)
        n.check(n.lib().rpsf_stars_label(self._handle, n._ptr(flags), n._ptr(labels)))
        return labels

    def info(self) -> tuple[int, int]:
        rows, cols = ctypes.c_int(0), ctypes.c_int(0)
        self._native.check(self._native.lib().rpsf_stars_info(self._handle, ctypes.byref(rows), ctypes.byref(cols)))
        return rows.value, cols.value

    def kernel_ms(self) -> tuple[float, float, float, float]:
        """Device time of the last S1, S2, S3 and S4 launches."""
        ms = (ctypes.c_double * 4)()
        self._native.check(self._native.lib().rpsf_stars_kernel_ms(self._handle, ms))
        return tuple(ms)

    def close(self) -> None:
        if self._handle is not None and self._handle.value:
            self._native.lib().rpsf_stars_destroy(self._handle)
            self._handle = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class _Model:
    """A native model handle: a cube of ``n_cells x N x N`` float64 values on the device, uploaded once (``rpsf_stars_model``)."""

    def __init__(self, values: np.ndarray, device: int = 0) -> None:
        from regularizepsf_amd import _native

        self._native = _native
        self.values = np.ascontiguousarray(values, np.float64)
        if self.values.ndim != 3 or self.values.shape[1] != self.values.shape[2]:
            msg = f"a model is a cube of n_cells x N x N values, not of shape {self.values.shape}"
            raise IncorrectShapeError(msg)
        self.size, self.device = int(self.values.shape[1]), int(device)
        self._handle = ctypes.c_void_p()
        _native.check(_native.lib().rpsf_stars_model_create(int(device), len(self.values), self.size, _native._ptr(self.values),
                                                            ctypes.byref(self._handle)))

    def close(self) -> None:
        if self._handle is not None and self._handle.value:
            self._native.lib().rpsf_stars_model_destroy(self._handle)
            self._handle = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def filter_mesh(level: np.ndarray, rms: np.ndarray) -> tuple[np.ndarray, np.ndarray, float] | None:
    """The host step between S1 and S2: boxes without a usable pixel take the median of the others, a 3 x 3 median filter runs
    over both meshes, and the global rms is the median of the filtered rms.  None when no box has a usable pixel."""
    from scipy.ndimage import median_filter

    valid = np.isfinite(level) & np.isfinite(rms)
    if not valid.any():
        return None
    level = np.where(valid, level, np.median(level[valid]))
    rms = np.where(valid, rms, np.median(rms[valid]))
    level, rms = median_filter(level, 3, mode="nearest"), median_filter(rms, 3, mode="nearest")
    return level, rms, float(np.median(rms))


def frame_stars(finder, frame: np.ndarray, mask: np.ndarray | None, threshold: float, min_area: int, max_area: int | None) -> np.ndarray:
    """One frame through a finder (anything with ``background`` and ``detect``): (k, 4) rows of (row, col, flux, area)."""
    level, rms = finder.background(frame, mask)
    filtered = filter_mesh(level, rms)
    if filtered is None:
        return np.zeros((0, 4))
    level, _, global_rms = filtered
    return finder.detect(level, threshold * global_rms, min_area, max_area)


def frame_stars_device(finder, frame, mask: np.ndarray | None, threshold: float, min_area: int, max_area: int | None) -> np.ndarray:
    """``frame_stars`` on the fused route: ``frame`` is a host array or a 2-D ``DeviceArray``; the mesh never leaves the device."""
    finder.background_device(frame, mask)
    return finder.detect_device(threshold, min_area, max_area)


def refine_sigma_option(refine_sigma) -> float | None:
    """``refine_sigma`` of the builder's ``finder_options``, range-checked: None or one window sigma."""
    if refine_sigma is None:
        return None
    if isinstance(refine_sigma, (bool, np.bool_)) or not isinstance(refine_sigma, (int, float, np.integer, np.floating)):
        msg = f"refine_sigma must be None or a number, not {refine_sigma!r}"
        raise TypeError(msg)
    if not MIN_SIGMA <= float(refine_sigma) <= MAX_SIGMA:
        msg = f"refine_sigma must lie in {MIN_SIGMA:g} ... {MAX_SIGMA:g}, got {refine_sigma}"
        raise ValueError(msg)
    return float(refine_sigma)


def refined_positions(positions: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """The positions the builder's ``refine_sigma`` option takes for its detections ``positions``: the refined one, and the detected one
    where the iteration stopped with ``NO_FLUX`` or ``RAN_AWAY``.  ``rows``: S7's rows for those positions, or ``refine_stars``' structured
    array of them."""
    positions = np.asarray(positions, np.float64).reshape(-1, 2)
    rows = np.asarray(rows)
    if rows.dtype.names is not None:
        flags, refined = rows["flags"].astype(np.int64), np.stack([rows["row"], rows["col"]], axis=-1).astype(np.float64)
    else:
        rows = np.asarray(rows, np.float64).reshape(-1, len(REFINE_COLUMNS))
        flags, refined = rows[:, REFINE_COLUMNS.index("flags")].astype(np.int64), rows[:, 2:4]
    failed = (flags & (NO_FLUX | RAN_AWAY)) != 0
    return np.ascontiguousarray(np.where(failed[:, None], positions, refined))


def refine_detections(finder, positions: np.ndarray, refine_sigma: float) -> np.ndarray:
    """S7 with its defaults and the finder's own background on the detections of the frame the finder holds (after a ``detect_device``):
    ``(k, 2)`` positions, ``refined_positions``' rule applied.  Nothing is launched for no detections."""
    positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
    if len(positions) == 0:
        return positions
    return refined_positions(positions, finder.refine(positions, refine_sigma))


def _masks(mask, frames: list, shape: tuple[int, int] | None = None) -> list[np.ndarray | None]:
    """One host mask (or None) per frame; ``shape``: what a mask must have when that is not the frames' (the scaled frames')."""
    if mask is None:
        return [None] * len(frames)
    if is_device_array(mask) or (isinstance(mask, (list, tuple)) and any(is_device_array(m) for m in mask)):
        msg = "masks are host arrays: a mask on the device is not supported, bring it to the host (to_host)"
        raise TypeError(msg)
    shape = tuple(frames[0].shape) if shape is None else shape
    if isinstance(mask, np.ndarray) and mask.ndim == 2:
        masks = [mask] * len(frames)
    else:
        masks = [np.asarray(m) for m in mask]
        if len(masks) != len(frames):
            msg = f"mask has {len(masks)} entries for {len(frames)} frames"
            raise ValueError(msg)
    for m in masks:
        if m.shape != shape:
            msg = f"A mask of shape {m.shape} does not fit frames of shape {shape}"
            raise IncorrectShapeError(msg)
    return [m.astype(bool) for m in masks]


def find_stars(images, threshold: float = 3.0, mask=None, *, box: int = 64, min_area: int = 5, max_area: int | None = None,
               deblend: bool = False, deblend_contrast: float = 0.005, deblend_prominence: float = 1.0,
               device: int = 0) -> list[np.ndarray]:
    """Star positions per frame, in the form ``ArrayPSFBuilder.build(..., stars=...)`` takes: a list of ``(k, 2)`` float64
    arrays of ``(row, col)``, one per frame; a frame without detections gives shape ``(0, 2)``.

    ``images``: what ``build`` takes (a 3-D array, a list of 2-D arrays, a generator, or one 2-D array), or frames that live on
    ``device``: a 2-D or 3-D ``DeviceArray`` or a list of 2-D ``DeviceArray`` s / objects with ``__cuda_array_interface__``, of the dtypes
    and strides ``apply`` takes - they are read where they lie, and the result is the host call's on the same values.  ``threshold``: in units
    of the frame's global background rms.  ``mask``: None, one 2-D boolean array for all frames or one per frame (True = ignore).
    ``box``: the background box in pixels, 8 ... 128.  A component is kept when ``min_area <= area <= max_area`` (None: no
    upper limit) and its background-subtracted flux is positive.  ``deblend``: split touching stars - inside each component every
    pixel ascends the filtered residual to a peak, and a peak's basin becomes an object of its own when its area is at least
    ``min_area``, its flux at least ``deblend_contrast`` (0 ... 1; ``sep``'s ``deblend_cont``) of the component's and its peak at least
    ``deblend_prominence`` thresholds above the saddle to its neighbours; the area and flux rule then applies per object.  Off (the
    default), every result is what it was.  Not ``sep``, and with ``deblend`` still not ``sep``'s multi-threshold tree: see the module
    docstring.
    """
    split = deblend_options(deblend, deblend_contrast, deblend_prominence)
    if not MIN_BOX <= int(box) <= MAX_BOX:
        msg = f"box must lie in {MIN_BOX} ... {MAX_BOX}, got {box}"
        raise ValueError(msg)
    frames = _device_frames(images, device)
    one_frame = frame_stars_device
    if frames is None:
        frames, one_frame = _frames(images), frame_stars
    masks = _masks(mask, frames)
    finder = _Finder(frames[0].shape, box, device)
    try:
        if split[0]:
            finder.set_deblend(*split)
        return [np.ascontiguousarray(one_frame(finder, frame, m, float(threshold), int(min_area), max_area)[:, :2])
                for frame, m in zip(frames, masks)]
    finally:
        finder.close()


def ellipse(rr: np.ndarray, cc: np.ndarray, rc: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``(a, b, theta, elongation)`` of central second moments, NumPy float64: the eigenvalues ``(rr + cc) / 2 +- sqrt(((rr - cc) / 2)^2
    + rc^2)``, ``a`` and ``b`` their square roots (NaN for a negative one), ``theta = atan2(2 rc, cc - rr) / 2`` - the major axis
    from the column axis towards the row axis, ``sep``'s ``theta`` with x = col and y = row - and ``elongation = a / b`` by IEEE rules."""
    rr, cc, rc = (np.asarray(v, np.float64) for v in (rr, cc, rc))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean, half = (rr + cc) / 2, np.sqrt(((rr - cc) / 2) ** 2 + rc ** 2)
        a, b = np.sqrt(mean + half), np.sqrt(mean - half)
        return a, b, 0.5 * np.arctan2(2 * rc, cc - rr), a / b


def catalog_from_shapes(shapes: np.ndarray) -> np.ndarray:
    """The structured catalogue (``CATALOG_DTYPE``) of S5's shape rows."""
    shapes = np.asarray(shapes, np.float64).reshape(-1, len(SHAPE_COLUMNS))
    out = np.empty(len(shapes), CATALOG_DTYPE)
    for j, name in enumerate(SHAPE_COLUMNS):
        out[name] = shapes[:, j]
    out["a"], out["b"], out["theta"], out["elongation"] = ellipse(out["rr"], out["cc"], out["rc"])
    return out


def star_catalog(images, threshold: float = 3.0, mask=None, *, box: int = 64, min_area: int = 5, max_area: int | None = None,
                 deblend: bool = False, deblend_contrast: float = 0.005, deblend_prominence: float = 1.0,
                 device: int = 0) -> list[np.ndarray]:
    """``find_stars`` with a catalogue per frame: a list of NumPy structured arrays, one per frame, with the float64 fields ``row, col,
    flux, area, peak, peak_row, peak_col, row_min, row_max, col_min, col_max, abs_flux, rr, cc, rc, a, b, theta, elongation``; a frame
    without detections gives length 0 with the same dtype.  The arguments are ``find_stars``'s, device frames included, and
    ``row, col`` are its positions bit for bit.

    For each detection, with ``P`` the pixels of its component (with ``deblend``: of its object), ``d`` the background-subtracted
    pixel, ``dr = r - row`` and ``dc = c - col``: ``rr = sum_P d dr^2 / flux``, ``cc = sum_P d dc^2 / flux``, ``rc = sum_P d dr dc /
    flux``, ``abs_flux = sum_P |d|``, ``peak = max_P d`` at ``(peak_row, peak_col)``, and the bounding box of ``P``.  ``a``, ``b``,
    ``theta`` and ``elongation`` are ``ellipse``'s: ``theta`` is the major axis measured from the column axis towards the row axis.
    ``b`` (and ``elongation``) is NaN where the smaller eigenvalue is negative, which a detected pixel with ``d < 0`` can cause.

    This is NOT ``sep``'s catalogue: no 1 / 12 pixel term, no clamp of a singular matrix, and the moments are taken over the detection
    footprint of this detector, which biases ``a`` and ``b`` low.  ``cat[cat["elongation"] < 1.5]`` goes to
    ``ArrayPSFBuilder.build(..., stars=...)`` as it is.
    """
    split = deblend_options(deblend, deblend_contrast, deblend_prominence)
    if not MIN_BOX <= int(box) <= MAX_BOX:
        msg = f"box must lie in {MIN_BOX} ... {MAX_BOX}, got {box}"
        raise ValueError(msg)
    frames = _device_frames(images, device)
    one_frame = frame_stars_device
    if frames is None:
        frames, one_frame = _frames(images), frame_stars
    masks = _masks(mask, frames)
    finder = _Finder(frames[0].shape, box, device)
    try:
        if split[0]:
            finder.set_deblend(*split)
        catalogs = []
        for frame, m in zip(frames, masks):
            rows = one_frame(finder, frame, m, float(threshold), int(min_area), max_area)
            # (no usable box at all: frame_stars returns before any detect, and there is nothing to measure)
            catalogs.append(catalog_from_shapes(finder.measure() if len(rows) else np.zeros((0, len(SHAPE_COLUMNS)))))
        return catalogs
    finally:
        finder.close()


# ---------------------------------------------------------------------------------------------------------------------- apertures
def photometry_columns(m: int) -> int:
    """The float64 per row of kernel S6 for ``m`` radii (``RPSF_STARS_PHOTOMETRY_COLUMNS``)."""
    return 2 + 3 * int(m) + len(PHOTOMETRY_SUMS)


def photometry_dtype(m: int) -> np.dtype:
    """The structured dtype of ``star_photometry`` for ``m`` radii: ``flux``, ``area`` and ``coverage`` are sub-arrays of shape ``(m,)``."""
    per_radius = {"flux", "area", "coverage"}
    names = ("row", "col", "flux", "area", "coverage", "abs_flux", "peak", "peak_row", "peak_col", "drow", "dcol", "rr", "cc", "rc", "a", "b",
             "theta", "elongation", "half_light_radius")
    return np.dtype([(name, np.float64, (int(m),)) if name in per_radius else (name, np.float64) for name in names])


def aperture_radii(radii) -> np.ndarray:
    """``radii`` as S6 takes them, range-checked: 1 ... 8 values, strictly ascending, ``0 < R <= 64``."""
    try:
        radii = np.atleast_1d(np.asarray(radii, np.float64))
    except (TypeError, ValueError) as error:
        msg = f"radii must be numbers, not {radii!r}"
        raise TypeError(msg) from error
    if radii.ndim != 1 or not 1 <= len(radii) <= MAX_RADII:
        msg = f"radii must be 1 ... {MAX_RADII} values, got shape {radii.shape}"
        raise ValueError(msg)
    if not np.all((radii > 0.0) & (radii <= MAX_RADIUS)):
        msg = f"radii must lie in 0 < R <= {MAX_RADIUS:g}, got {radii.tolist()}"
        raise ValueError(msg)
    if np.any(np.diff(radii) <= 0.0):
        msg = f"radii must ascend strictly, got {radii.tolist()}"
        raise ValueError(msg)
    return np.ascontiguousarray(radii)


def half_light_radius(radii: np.ndarray, flux: np.ndarray) -> np.ndarray:
    """Per row of ``flux`` ((k, m), the curve of growth at ``radii``): the radius where the piecewise-linear curve through ``(0, 0)`` and
    ``(R_k, flux_k)`` first reaches half of the outermost flux ``F``; NaN where ``F <= 0`` or ``F`` is not finite."""
    radii, flux = np.asarray(radii, np.float64), np.asarray(flux, np.float64).reshape(-1, len(radii))
    total = flux[:, -1]
    good = np.isfinite(total) & (total > 0.0)
    half = np.where(good, total / 2, np.nan)
    out, open_ = np.full(len(flux), np.nan), good.copy()
    r_before, f_before = 0.0, np.zeros(len(flux))
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, r in enumerate(radii):
            here = open_ & (flux[:, k] >= half)  # f_before < half <= flux_k: the segment crosses, and its slope is positive
            out[here] = r_before + (half[here] - f_before[here]) * (r - r_before) / (flux[here, k] - f_before[here])
            open_ &= ~here
            r_before, f_before = r, flux[:, k]
    return out


def photometry_from_sums(rows: np.ndarray, radii, subpix: int) -> np.ndarray:
    """The structured result (``photometry_dtype``) of S6's rows, everything derived in NumPy float64: ``area = N_use / s^2``, ``coverage =
    N_use / N_all`` (0 / 0 = NaN), ``drow = mr / F`` and ``dcol = mc / F`` with ``F`` the outermost flux, ``rr = mrr / F - drow^2`` (``cc``,
    ``rc`` alike), the ellipse of ``ellipse`` and ``half_light_radius``."""
    radii = np.asarray(radii, np.float64).ravel()
    m = len(radii)
    rows = np.asarray(rows, np.float64).reshape(-1, photometry_columns(m))
    out = np.empty(len(rows), photometry_dtype(m))
    out["row"], out["col"] = rows[:, 0], rows[:, 1]
    flux, n_use, n_all = rows[:, 2:2 + m], rows[:, 2 + m:2 + 2 * m], rows[:, 2 + 2 * m:2 + 3 * m]
    sums = {name: rows[:, 2 + 3 * m + j] for j, name in enumerate(PHOTOMETRY_SUMS)}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["flux"], out["area"], out["coverage"] = flux, n_use / float(subpix * subpix), n_use / n_all
        for name in ("abs_flux", "peak", "peak_row", "peak_col"):
            out[name] = sums[name]
        total = flux[:, -1]
        drow, dcol = sums["mr"] / total, sums["mc"] / total
        out["drow"], out["dcol"] = drow, dcol
        out["rr"], out["cc"], out["rc"] = sums["mrr"] / total - drow * drow, sums["mcc"] / total - dcol * dcol, sums["mrc"] / total - drow * dcol
    out["a"], out["b"], out["theta"], out["elongation"] = ellipse(out["rr"], out["cc"], out["rc"])
    out["half_light_radius"] = half_light_radius(radii, flux)
    return out


def star_photometry(images, stars, radii, mask=None, *, background: str = "mesh", box: int = 64, subpix: int = 5,
                    device: int = 0) -> list[np.ndarray]:
    """Forced aperture photometry at given positions: a list of NumPy structured arrays, one per frame and one row per position, with the
    float64 fields ``row, col, flux (m,), area (m,), coverage (m,), abs_flux, peak, peak_row, peak_col, drow, dcol, rr, cc, rc, a, b,
    theta, elongation, half_light_radius`` for ``m = len(radii)``.

    ``images``: what ``find_stars`` takes, device frames included.  ``stars``: what ``build(..., stars=)`` takes - per frame a ``(k, 2)``
    array of ``(row, col)`` or a structured array with those fields (``star_catalog``'s, whole or filtered); positions are finite with
    ``|row|, |col| < 2^20`` and may lie off the frame.  ``radii``: 1 ... 8 aperture radii in pixels, strictly ascending, ``0 < R <= 64``.
    ``mask``: as for ``find_stars``.  ``background``: ``"mesh"`` subtracts ``find_stars``' background surface (``box``: its box), ``"none"``
    takes the pixels as they are, for frames that are already background-subtracted (the mesh kernels S1 and S1b still run then; their
    result is not read).  ``subpix`` = ``s``, 1 ... 8: every pixel is sampled on an ``s x s`` lattice.

    A sub-sample of pixel ``(r, c)`` at offsets ``o_a = (2a + 1 - s) / (2s)`` lies in aperture ``k`` when ``(r - row + o_a)^2 + (c - col +
    o_b)^2 <= R_k^2``, and the pixel's weight ``w_k`` is the fraction of its ``s^2`` sub-samples that do.  With ``d`` the background-subtracted
    pixel: ``flux[k] = sum w_k d`` over usable (finite, unmasked) pixels of the frame, ``area[k]`` the sum of their ``w_k``, ``coverage[k]``
    that area over the aperture's whole area, off-frame part included (0 for an aperture wholly off the frame).  On the outermost aperture,
    with ``F = flux[-1]``: ``abs_flux = sum w |d|``, ``peak`` the largest ``d`` at ``(peak_row, peak_col)`` (NaN at (-1, -1) without a
    usable pixel), ``(drow, dcol) = sum w d (r - row, c - col) / F`` the centroid's offset from the given position, ``rr, cc, rc`` the
    central second moments ``sum w d (r - row)^2 / F - drow^2`` etc. and ``a, b, theta, elongation`` as in ``star_catalog``.
    ``half_light_radius``: where the piecewise-linear curve of growth through ``(0, 0)`` and ``(R_k, flux[k])`` first reaches ``F / 2``;
    NaN when ``F <= 0`` or not finite.  With ``background="mesh"`` a frame without a usable pixel has no background: every flux and
    moment is NaN, the areas are delivered.

    This is NOT ``sep``'s ``sum_circle`` / ``flux_radius``: the comparison is ``<=`` on this lattice, there is no error column and no
    1 / 12 term, and masked pixels are excluded and reported through ``coverage``, not corrected for.
    """
    if background not in ("mesh", "none"):
        msg = f'background must be "mesh" or "none", not {background!r}'
        raise ValueError(msg)
    if not MIN_BOX <= int(box) <= MAX_BOX:
        msg = f"box must lie in {MIN_BOX} ... {MAX_BOX}, got {box}"
        raise ValueError(msg)
    if isinstance(subpix, (bool, np.bool_)) or not isinstance(subpix, (int, np.integer)):
        msg = f"subpix must be an integer, not {subpix!r}"
        raise TypeError(msg)
    if not 1 <= subpix <= MAX_SUBPIX:
        msg = f"subpix must lie in 1 ... {MAX_SUBPIX}, got {subpix}"
        raise ValueError(msg)
    radii = aperture_radii(radii)
    frames = _device_frames(images, device)
    if frames is None:
        frames = _frames(images)
    if isinstance(stars, np.ndarray) and (stars.dtype.names is not None or stars.ndim == 2):
        stars = [stars]  # one frame's stars, as they are
    if len(stars) != len(frames):
        msg = f"stars has {len(stars)} entries for {len(frames)} frames"
        raise ValueError(msg)
    positions = [np.ascontiguousarray(star_positions(s)) for s in stars]
    for i, p in enumerate(positions):
        if not np.all(np.abs(p) < MAX_COORD):  # (false for NaN)
            msg = f"stars[{i}] has a position that is not finite or not inside |row|, |col| < 2^20"
            raise ValueError(msg)
    masks = _masks(mask, frames)
    finder = _Finder(frames[0].shape, box, device)
    try:
        out = []
        for frame, m, p in zip(frames, masks, positions):
            finder.background_device(frame, m)
            out.append(photometry_from_sums(finder.photometry(p, radii, subpix, background == "mesh"), radii, subpix))
        return out
    finally:
        finder.close()


# ---------------------------------------------------------------------------------------------------------------------- windowed positions
REFINE_FIELDS = ("row", "col", "row0", "col0", "sigma", "niter", "flags", "converged", "step_row", "step_col", "flux", "abs_flux", "coverage",
                 "drow", "dcol", "wrr", "wcc", "wrc", "rr", "cc", "rc", "a", "b", "theta", "elongation")


def refine_dtype() -> np.dtype:
    """The structured dtype of ``refine_stars``: float64 fields but for ``niter`` and ``flags`` (int32) and ``converged`` (bool)."""
    kinds = {"niter": np.int32, "flags": np.int32, "converged": np.bool_}
    return np.dtype([(name, kinds.get(name, np.float64)) for name in REFINE_FIELDS])


def window_corrected(wrr, wcc, wrc, sigma) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(rr, cc, rc)``: the matrix ``(M_w^-1 - I / sigma^2)^-1`` of the windowed central moments ``M_w = [[wrr, wrc], [wrc, wcc]]``, NumPy
    float64, where that difference is positive definite; NaN otherwise.  A Gaussian source of covariance ``M`` seen through a Gaussian
    window of ``sigma`` has ``M_w^-1 = M^-1 + I / sigma^2``: the correction is exact for a Gaussian under the continuous, untruncated
    window, and only there."""
    wrr, wcc, wrc, sigma = (np.asarray(v, np.float64) for v in (wrr, wcc, wrc, sigma))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        det_w = wrr * wcc - wrc * wrc
        inv = 1.0 / (sigma * sigma)
        drr, dcc, drc = wcc / det_w - inv, wrr / det_w - inv, -wrc / det_w  # M_w^-1 - I / sigma^2
        det = drr * dcc - drc * drc
        good = (drr > 0.0) & (det > 0.0) & np.isfinite(det)
        rr, cc, rc = dcc / det, drr / det, -drc / det
    nan = np.float64(np.nan)
    return np.where(good, rr, nan), np.where(good, cc, nan), np.where(good, rc, nan)


def refine_from_sums(rows: np.ndarray) -> np.ndarray:
    """The structured result (``refine_dtype``) of S7's rows, everything derived in NumPy float64: ``coverage = N_use / N_all``, ``drow = mr /
    S`` and ``dcol = mc / S`` (what is left of the offset at the position returned), the windowed central moments ``wrr = mrr / S -
    drow^2`` (``wcc``, ``wrc`` alike), ``rr, cc, rc`` by ``window_corrected``, the ellipse of ``ellipse`` on those, and ``converged = flags
    == 0 and niter > 0``."""
    rows = np.asarray(rows, np.float64).reshape(-1, len(REFINE_COLUMNS))
    col = {name: rows[:, j] for j, name in enumerate(REFINE_COLUMNS)}
    out = np.empty(len(rows), refine_dtype())
    for name in ("row", "col", "row0", "col0", "sigma", "step_row", "step_col", "flux", "abs_flux"):
        out[name] = col[name]
    out["niter"], out["flags"] = col["niter"].astype(np.int32), col["flags"].astype(np.int32)
    out["converged"] = (out["flags"] == 0) & (out["niter"] > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        total = col["flux"]
        out["coverage"] = col["n_use"] / col["n_all"]
        drow, dcol = col["mr"] / total, col["mc"] / total
        out["drow"], out["dcol"] = drow, dcol
        out["wrr"], out["wcc"], out["wrc"] = col["mrr"] / total - drow * drow, col["mcc"] / total - dcol * dcol, col["mrc"] / total - drow * dcol
    out["rr"], out["cc"], out["rc"] = window_corrected(out["wrr"], out["wcc"], out["wrc"], out["sigma"])
    out["a"], out["b"], out["theta"], out["elongation"] = ellipse(out["rr"], out["cc"], out["rc"])
    return out


def _refine_sigmas(sigma, counts: list[int]) -> list[np.ndarray]:
    """``sigma`` of ``refine_stars`` as one float64 array per frame: a scalar, one array for all frames, or a list with one entry (a scalar
    or an array) per frame."""
    per_frame = isinstance(sigma, (list, tuple)) and any(np.ndim(s) > 0 for s in sigma)
    if per_frame and len(sigma) != len(counts):
        msg = f"sigma has {len(sigma)} entries for {len(counts)} frames"
        raise ValueError(msg)
    out = []
    for i, k in enumerate(counts):
        try:
            one = np.asarray(sigma[i] if per_frame else sigma, np.float64)
        except (TypeError, ValueError) as error:
            msg = f"sigma must be numbers, not {sigma!r}"
            raise TypeError(msg) from error
        if one.ndim > 1 or (one.ndim == 1 and len(one) != k):
            msg = f"sigma has shape {one.shape} for the {k} stars of frame {i}: a scalar or one value per star"
            raise ValueError(msg)
        one = np.ascontiguousarray(np.broadcast_to(one, (k,)))
        if not np.all((one >= MIN_SIGMA) & (one <= MAX_SIGMA)):  # (false for NaN)
            msg = f"sigma must lie in {MIN_SIGMA:g} ... {MAX_SIGMA:g}"
            raise ValueError(msg)
        out.append(one)
    return out


def refine_stars(images, stars, sigma, mask=None, *, background: str = "mesh", box: int = 64, max_iter: int = 16, eps: float = 1e-4,
                 max_shift: float = 2.0, device: int = 0) -> list[np.ndarray]:
    """Gaussian-windowed positions and moments at given positions (SExtractor's ``XWIN`` iteration): a list of NumPy structured arrays
    (``refine_dtype``), one per frame and one row per position, with the fields ``row, col`` (the refined position), ``row0, col0`` (the
    input), ``sigma, niter, flags, converged, step_row, step_col, flux, abs_flux, coverage, drow, dcol, wrr, wcc, wrc, rr, cc, rc, a, b,
    theta, elongation``.  ``build(..., stars=refine_stars(...))`` and ``star_photometry(frames, refine_stars(...), radii)`` take it as it is.

    ``images``, ``stars``, ``mask``, ``background`` and ``box`` are ``star_photometry``'s.  ``sigma``: the window's sigma in pixels, 0.5 ...
    16 - a scalar, one array for all frames (one value per star), or a list with one array per frame; the star's own sigma is the usual
    choice.  ``max_iter``: 0 ... 64; 0 measures at the given positions.  ``eps > 0``: the iteration has converged when a step ``(dy, dx)`` has
    ``dy^2 + dx^2 < eps^2``.  ``max_shift``: ``0 < max_shift <= 64``, the farthest a position may move from its start.

    One walk at ``p = (row, col)``: over the pixels with ``q = (r - row)^2 + (c - col)^2 <= (4 sigma)^2``, usable (finite, unmasked, on
    the frame), with ``d`` the background-subtracted pixel and ``w = exp(-q / (2 sigma^2))`` (this package's own ``exp`` in plain float64
    arithmetic, the same bits on the GPU and on the CPU): ``S = sum w d``, ``A = sum w |d|`` and the first and second moments of ``w d``
    around ``p``.  From the given position: walk; without flux (``S <= 0`` or not finite) stop with flag ``NO_FLUX`` (1); step ``p' = p + 2
    (mr, mc) / S``; if ``p'`` is farther than ``max_shift`` from the start, stop with ``RAN_AWAY`` (2) at ``p``; else accept it, and stop
    when the step is below ``eps`` (converged) or after ``max_iter`` steps (``NOT_CONVERGED``, 4).  ``step_row, step_col`` are the last step
    computed (NaN if none), ``niter`` the steps accepted.  One more walk at the position returned gives ``flux = S``, ``abs_flux = A``,
    ``coverage`` (the usable share of the window's pixels), ``drow, dcol`` (the offset that is left), the windowed central moments
    ``wrr, wcc, wrc``, and ``rr, cc, rc``: those corrected for the window, ``(M_w^-1 - I / sigma^2)^-1``, NaN where that difference is not
    positive definite; ``a, b, theta, elongation`` as in ``star_catalog``, of the corrected moments.  ``converged`` is ``flags == 0 and
    niter > 0``.  With ``background="mesh"`` a frame without a usable pixel has no background: every position stays, flagged ``NO_FLUX``,
    with NaN sums.

    The correction is exact for a Gaussian source under the continuous, untruncated window only.  This is NOT ``sep``'s ``winpos``: no
    sub-pixel sampling of the window's rim, the comparison is ``<=``, there is no error column, and masked pixels are excluded and
    reported through ``coverage``, not corrected for.
    """
    if background not in ("mesh", "none"):
        msg = f'background must be "mesh" or "none", not {background!r}'
        raise ValueError(msg)
    if not MIN_BOX <= int(box) <= MAX_BOX:
        msg = f"box must lie in {MIN_BOX} ... {MAX_BOX}, got {box}"
        raise ValueError(msg)
    if isinstance(max_iter, (bool, np.bool_)) or not isinstance(max_iter, (int, np.integer)):
        msg = f"max_iter must be an integer, not {max_iter!r}"
        raise TypeError(msg)
    if not 0 <= max_iter <= MAX_ITER:
        msg = f"max_iter must lie in 0 ... {MAX_ITER}, got {max_iter}"
        raise ValueError(msg)
    if not (float(eps) > 0.0 and np.isfinite(eps)):
        msg = f"eps must be positive and finite, got {eps}"
        raise ValueError(msg)
    if not 0.0 < float(max_shift) <= MAX_RADIUS:
        msg = f"max_shift must lie in 0 < max_shift <= {MAX_RADIUS:g}, got {max_shift}"
        raise ValueError(msg)
    frames = _device_frames(images, device)
    if frames is None:
        frames = _frames(images)
    if isinstance(stars, np.ndarray) and (stars.dtype.names is not None or stars.ndim == 2):
        stars = [stars]  # one frame's stars, as they are
    if len(stars) != len(frames):
        msg = f"stars has {len(stars)} entries for {len(frames)} frames"
        raise ValueError(msg)
    positions = [np.ascontiguousarray(star_positions(s)) for s in stars]
    for i, p in enumerate(positions):
        if not np.all(np.abs(p) < MAX_COORD):  # (false for NaN)
            msg = f"stars[{i}] has a position that is not finite or not inside |row|, |col| < 2^20"
            raise ValueError(msg)
    sigmas = _refine_sigmas(sigma, [len(p) for p in positions])
    masks = _masks(mask, frames)
    finder = _Finder(frames[0].shape, box, device)
    try:
        out = []
        for frame, m, p, sg in zip(frames, masks, positions, sigmas):
            finder.background_device(frame, m)
            out.append(refine_from_sums(finder.refine(p, sg, max_iter, eps, max_shift, background == "mesh")))
        return out
    finally:
        finder.close()


# ---------------------------------------------------------------------------------------------------------------------- model fits
FIT_FIELDS = ("row", "col", "cell", "flags", "flux", "background", "n_use", "n_all", "coverage", "dof", "chi2", "rms", "abs_res",
              "residual_fraction", "peak_res", "peak_e", "peak_row", "peak_col", "sm", "sm_all", "smm", "sd", "sdm", "sdd", "no_mesh", "too_few",
              "degenerate", "bad_cell")


def fit_dtype() -> np.dtype:
    """The structured dtype of ``fit_stars``: float64 fields but for ``cell``, ``flags``, ``n_use``, ``n_all`` and ``dof`` (int32) and the four
    booleans of the flags."""
    kinds = {"cell": np.int32, "flags": np.int32, "n_use": np.int32, "n_all": np.int32, "dof": np.int32, "no_mesh": np.bool_,
             "too_few": np.bool_, "degenerate": np.bool_, "bad_cell": np.bool_}
    return np.dtype([(name, kinds.get(name, np.float64)) for name in FIT_FIELDS])


def fit_from_sums(rows: np.ndarray, fit_background: bool = True) -> np.ndarray:
    """The structured result (``fit_dtype``) of S8's rows, everything derived in NumPy float64: ``coverage = Sm / Sm_all``, ``dof = n - 2``
    (``n - 1`` without a fitted background), ``rms = sqrt(chi2 / dof)`` (NaN when ``dof <= 0``), ``residual_fraction = abs_res / (|flux|
    |Sm|)`` and one boolean per flag."""
    rows = np.asarray(rows, np.float64).reshape(-1, len(FIT_COLUMNS))
    col = {name: rows[:, j] for j, name in enumerate(FIT_COLUMNS)}
    out = np.empty(len(rows), fit_dtype())
    for name in ("row", "col", "flux", "background", "chi2", "abs_res", "peak_res", "peak_e", "peak_row", "peak_col", "sm", "sm_all", "smm", "sd",
                 "sdm", "sdd"):
        out[name] = col[name]
    for name in ("cell", "flags", "n_use", "n_all"):
        out[name] = col[name].astype(np.int32)
    out["dof"] = out["n_use"] - (2 if fit_background else 1)
    for name, bit in (("no_mesh", NO_MESH), ("too_few", TOO_FEW), ("degenerate", DEGENERATE), ("bad_cell", BAD_CELL)):
        out[name] = (out["flags"] & bit) != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        dof = out["dof"].astype(np.float64)
        out["coverage"] = col["sm"] / col["sm_all"]
        out["rms"] = np.where(dof > 0, np.sqrt(col["chi2"] / np.where(dof > 0, dof, np.nan)), np.nan)
        out["residual_fraction"] = col["abs_res"] / (np.abs(col["flux"]) * np.abs(col["sm"]))
    return out


def nearest_cells(positions: np.ndarray, coordinates, size: int) -> np.ndarray:
    """Per position the index of the cell whose centre ``corner + N / 2`` is nearest in squared Euclidean distance ``(row - cy)^2 + (col -
    cx)^2``, float64; among equals the first in the order of ``coordinates``.  (k,) int32.  Many cells are searched through a k-d tree, which
    only proposes the candidates: every cell within the nearest one's distance (and a little beyond) is compared by the formula above."""
    positions = np.asarray(positions, np.float64).reshape(-1, 2)
    centres = np.asarray(coordinates, np.float64).reshape(-1, 2) + size / 2
    if len(positions) == 0:
        return np.zeros(0, np.int32)
    if len(centres) <= 64:
        candidates = np.broadcast_to(np.arange(len(centres)), (len(positions), len(centres)))
    else:
        from scipy.spatial import cKDTree

        tree = cKDTree(centres)
        nearest = tree.query(positions)[0]
        found = tree.query_ball_point(positions, nearest * (1 + 1e-9) + 1e-9, return_sorted=True)  # every cell that can be the nearest or tie
        counts = np.array([len(f) for f in found])
        flat, starts = np.concatenate([np.asarray(f, np.int64) for f in found]), np.cumsum(counts) - counts
        # ascending indices per position, the last one repeated up to the longest list: argmin takes the first of equals
        candidates = flat[starts[:, None] + np.minimum(np.arange(counts.max())[None, :], counts[:, None] - 1)]
    dy, dx = positions[:, 0, None] - centres[candidates, 0], positions[:, 1, None] - centres[candidates, 1]
    return candidates[np.arange(len(positions)), np.argmin(dy * dy + dx * dx, axis=1)].astype(np.int32)


def model_cube(psf) -> tuple[list, np.ndarray]:
    """``(coordinates, values)`` of an ``ArrayPSF`` or an ``IndexedCube`` of real values: the values as a C-contiguous float64 cube of
    ``n_cells x N x N``, ``4 <= N <= 256``, NaN cells (``build``'s cells without a star) as they are."""
    if not (hasattr(psf, "coordinates") and hasattr(psf, "values")):
        msg = f"psf must be an ArrayPSF or an IndexedCube, not {type(psf).__name__}"
        raise TypeError(msg)
    values = np.asarray(psf.values)
    if np.iscomplexobj(values) or values.dtype.kind not in "fiu":
        msg = f"the model's values must be real numbers, not {values.dtype}"
        raise TypeError(msg)
    if values.ndim != 3 or values.shape[1] != values.shape[2] or not MIN_MODEL <= values.shape[1] <= MAX_MODEL or len(values) == 0:
        msg = f"the model must be a cube of at least one cell of N x N values with {MIN_MODEL} <= N <= {MAX_MODEL}, not of shape {values.shape}"
        raise IncorrectShapeError(msg)
    return list(psf.coordinates), np.ascontiguousarray(values, np.float64)


def _fit_inputs(images, stars, psf, radius, mask, background, box, fit_background, cells, device) -> tuple:
    """What ``fit_stars`` and ``fit_positions`` make of their common arguments: ``(frames, masks, positions, cells, values, radius)``, one
    entry per frame in the first four."""
    if background not in ("mesh", "none"):
        msg = f'background must be "mesh" or "none", not {background!r}'
        raise ValueError(msg)
    if not MIN_BOX <= int(box) <= MAX_BOX:
        msg = f"box must lie in {MIN_BOX} ... {MAX_BOX}, got {box}"
        raise ValueError(msg)
    if not isinstance(fit_background, (bool, np.bool_)):
        msg = f"fit_background must be True or False, not {fit_background!r}"
        raise TypeError(msg)
    coordinates, values = model_cube(psf)
    size = values.shape[1]
    try:
        radius = float(radius)
    except (TypeError, ValueError) as error:
        msg = f"radius must be a number, not {radius!r}"
        raise TypeError(msg) from error
    limit = min(MAX_RADIUS, size / 2 - 1)
    if not 0.0 < radius <= limit:
        msg = f"radius must lie in 0 < R <= min({MAX_RADIUS:g}, N / 2 - 1) = {limit:g} for cells of {size}, got {radius}"
        raise ValueError(msg)
    frames = _device_frames(images, device)
    if frames is None:
        frames = _frames(images)
    if isinstance(stars, np.ndarray) and (stars.dtype.names is not None or stars.ndim == 2):
        stars = [stars]  # one frame's stars, as they are
    if len(stars) != len(frames):
        msg = f"stars has {len(stars)} entries for {len(frames)} frames"
        raise ValueError(msg)
    positions = [np.ascontiguousarray(star_positions(s)) for s in stars]
    for i, p in enumerate(positions):
        if not np.all(np.abs(p) < MAX_COORD):  # (false for NaN)
            msg = f"stars[{i}] has a position that is not finite or not inside |row|, |col| < 2^20"
            raise ValueError(msg)
    if cells is None:
        cells = [nearest_cells(p, coordinates, size) for p in positions]
    else:
        if isinstance(cells, np.ndarray) and cells.ndim == 1 and len(frames) == 1:
            cells = [cells]
        if len(cells) != len(frames):
            msg = f"cells has {len(cells)} entries for {len(frames)} frames"
            raise ValueError(msg)
        given, cells = cells, []
        for i, (c, p) in enumerate(zip(given, positions)):
            c = np.asarray(c)
            if c.dtype.kind not in "iu" and c.size:
                msg = f"cells[{i}] must be integers, not {c.dtype}"
                raise TypeError(msg)
            if c.shape != (len(p),):
                msg = f"cells[{i}] has shape {c.shape} for the {len(p)} stars of frame {i}"
                raise ValueError(msg)
            if c.size and (c.min() < -(2 ** 31) or c.max() >= 2 ** 31):
                msg = f"cells[{i}] has an index outside int32"
                raise ValueError(msg)
            cells.append(np.ascontiguousarray(c, np.int32))
    return frames, _masks(mask, frames), positions, cells, values, radius


@contextlib.contextmanager
def _fit_session(frames, masks, positions, cells, values, box: int, device: int):
    """One finder and one model for the frames of a fit: yields ``(finder, model, frames)``, where ``frames`` gives ``(k, positions,
    cells)`` of frame k once the finder holds that frame and its mesh.  Both handles are closed when the block is left, by a return or by an error."""
    finder = _Finder(frames[0].shape, box, device)
    model = None
    try:
        model = _Model(values, device)

        def each_frame():
            for k, (frame, m, p, c) in enumerate(zip(frames, masks, positions, cells)):
                finder.background_device(frame, m)
                yield k, p, c

        yield finder, model, each_frame()
    finally:
        if model is not None:
            model.close()
        finder.close()


def fit_stars(images, stars, psf, radius: float, mask=None, *, background: str = "mesh", box: int = 64, fit_background: bool = True,
              cells=None, device: int = 0) -> list[np.ndarray]:
    """Fit every star with the cell of a PSF model it belongs to and report the residual: a list of NumPy structured arrays
    (``fit_dtype``), one per frame and one row per position, with the fields ``row, col, cell, flags, flux, background, n_use, n_all,
    coverage, dof, chi2, rms, abs_res, residual_fraction, peak_res, peak_e, peak_row, peak_col``, the raw sums ``sm, sm_all, smm, sd, sdm,
    sdd`` and the booleans ``no_mesh, too_few, degenerate, bad_cell``.  On the frames a model was built from it says whether the model
    describes its stars, cell by cell; on frames after ``apply``, with the target PSF as the model, whether the correction worked.

    ``images``, ``stars``, ``mask``, ``background`` and ``box`` are ``star_photometry``'s, device frames included; ``refine_stars``' output and
    catalogues are taken by ``row`` / ``col``.  ``psf``: an ``ArrayPSF`` (``ArrayPSFBuilder.build``'s) or an ``IndexedCube`` of real
    values, cells of ``N x N`` with ``4 <= N <= 256``; it is uploaded once.  ``radius`` = ``R``: ``0 < R <= min(64, N / 2 - 1)``, the disc
    the fit sees.  ``fit_background``: fit a constant beside the flux.  ``cells``: None, or one integer array per frame (one array for a
    single frame) with the cell index of every star in the order of ``psf.coordinates``; None takes, per star, the cell whose centre ``corner
    + N / 2`` is nearest (squared Euclidean distance in float64; the first such cell in the cube's coordinate order wins a tie).

    A cell holds a star the way ``build`` cuts it: its centre at index ``h = N / 2 - 0.5`` on both axes.  The model at pixel ``(r, c)`` is
    the bilinear interpolation of the cell at ``(r - row + h, c - col + h)``.  Over the usable pixels (finite, unmasked, on the frame) with
    ``(r - row)^2 + (c - col)^2 <= R^2``, with ``d`` the background-subtracted pixel and ``m`` the model: ``n_use``, ``sm = sum m``, ``smm =
    sum m^2``, ``sd = sum d``, ``sdm = sum d m``, ``sdd = sum d^2``; ``n_all`` and ``sm_all`` take the whole disc, usable or not, and
    ``coverage = sm / sm_all`` is the share of the model the fit saw.  With ``fit_background``: ``D = n smm - sm^2``, ``flux = (n sdm - sm
    sd) / D``, ``background = (sd - flux sm) / n``; without: ``flux = sdm / smm``, ``background = 0``.  Then, with ``e = d - (flux m +
    background)``: ``chi2 = sum e^2``, ``abs_res = sum |e|``, ``peak_res = max |e|`` with its signed value ``peak_e`` at ``(peak_row,
    peak_col)``; ``dof = n_use - 2`` (``- 1`` without a fitted background), ``rms = sqrt(chi2 / dof)`` (NaN when ``dof <= 0``) and
    ``residual_fraction = abs_res / (|flux| |sm|)``, the residual's share of the fitted star.  Flags: ``NO_MESH`` (1: ``background="mesh"`` on
    a frame without a usable pixel), ``TOO_FEW`` (2: ``n_use < 3``, or ``< 1`` without a fitted background), ``DEGENERATE`` (4: ``D``, or
    ``smm``, not finite or ``<= 0`` - an all-zero cell, a cell of NaN as ``build`` leaves where it had no star, or a constant one with
    ``fit_background``), ``BAD_CELL`` (8: a cell index outside the
    model); with any of them ``flux``, ``background`` and the residual's columns are NaN.

    This is NOT a PSF-photometry package's fit: the weights are uniform - there is no error column and no variance weighting -, the position
    is given and not fitted (``refine_stars`` supplies positions), the interpolation is bilinear and does not conserve flux below the pixel
    scale, and masked pixels are excluded and reported through ``coverage``, not corrected for.
    """
    frames, masks, positions, cells, values, radius = _fit_inputs(images, stars, psf, radius, mask, background, box, fit_background, cells,
                                                                  device)
    with _fit_session(frames, masks, positions, cells, values, box, device) as (finder, model, each_frame):
        return [fit_from_sums(finder.fit(model, p, c, radius, bool(fit_background), background == "mesh"), bool(fit_background))
                for _, p, c in each_frame]


# ---------------------------------------------------------------------------------------------------------------------- weighted fits
WEIGHTED_FIT_FIELDS = (*FIT_FIELDS, "sw", "swm", "flux_err", "background_err", "flux_background_cov", "snr", "chi2_reduced")


def weighted_fit_dtype() -> np.dtype:
    """The structured dtype of ``fit_stars_weighted``: ``fit_dtype``'s fields with their kinds, then ``sw, swm, flux_err, background_err,
    flux_background_cov, snr, chi2_reduced`` (float64)."""
    kinds = {name: fit_dtype()[name] for name in FIT_FIELDS}
    return np.dtype([(name, kinds.get(name, np.float64)) for name in WEIGHTED_FIT_FIELDS])


def weighted_fit_from_sums(rows: np.ndarray, fit_background: bool = True) -> np.ndarray:
    """The structured result (``weighted_fit_dtype``) of S12's rows, everything derived in NumPy float64: ``fit_from_sums``' ``coverage``,
    ``dof``, ``residual_fraction`` and booleans; ``smm, sd, sdm, sdd`` are the weighted sums ``sum w m m, sum w d, sum w d m, sum w d d``;
    ``flux_err = sqrt(var_flux)``, ``background_err = sqrt(var_background)``, ``flux_background_cov``, ``snr = flux / flux_err``,
    ``chi2_reduced = chi2 / dof`` (NaN when ``dof <= 0``) and ``rms = sqrt(chi2_reduced)``."""
    rows = np.asarray(rows, np.float64).reshape(-1, len(FITW_COLUMNS))
    col = {name: rows[:, j] for j, name in enumerate(FITW_COLUMNS)}
    out = np.empty(len(rows), weighted_fit_dtype())
    for name in ("row", "col", "flux", "background", "chi2", "abs_res", "peak_res", "peak_e", "peak_row", "peak_col", "sm", "sm_all", "sw", "swm"):
        out[name] = col[name]
    for name, source in (("smm", "swmm"), ("sd", "swd"), ("sdm", "swdm"), ("sdd", "swdd"), ("flux_background_cov", "cov")):
        out[name] = col[source]
    for name in ("cell", "flags", "n_use", "n_all"):
        out[name] = col[name].astype(np.int32)
    out["dof"] = out["n_use"] - (2 if fit_background else 1)
    for name, bit in (("no_mesh", NO_MESH), ("too_few", TOO_FEW), ("degenerate", DEGENERATE), ("bad_cell", BAD_CELL)):
        out[name] = (out["flags"] & bit) != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        dof = out["dof"].astype(np.float64)
        out["coverage"] = col["sm"] / col["sm_all"]
        out["chi2_reduced"] = np.where(dof > 0, col["chi2"] / np.where(dof > 0, dof, np.nan), np.nan)
        out["rms"] = np.sqrt(out["chi2_reduced"])
        out["residual_fraction"] = col["abs_res"] / (np.abs(col["flux"]) * np.abs(col["sm"]))
        out["flux_err"] = np.sqrt(col["var_flux"])
        out["background_err"] = np.sqrt(col["var_background"])
        out["snr"] = col["flux"] / out["flux_err"]
    return out


def _variance_frames(variance, frames: list, device: int) -> list:
    """One variance frame per frame of ``frames``: host arrays for host frames, 2-D ``DeviceArray`` s for device frames."""
    from regularizepsf_amd.device_array import as_device_array

    on_device = not isinstance(frames[0], np.ndarray)
    shape = tuple(frames[0].shape)
    many = isinstance(variance, (list, tuple))
    given = list(variance) if many else [variance]
    if not given:
        msg = "variance is an empty list"
        raise ValueError(msg)
    if any(is_device_array(v) for v in given) != on_device or (on_device and not all(is_device_array(v) for v in given)):
        msg = ("variance and images must live in the same place: host arrays with host frames, device arrays with device frames "
               "(to_host / to_device bring one to the other)")
        raise TypeError(msg)
    if on_device:
        given = [as_device_array(v, device, what="variance") for v in given]
    else:
        given = [np.asarray(v) for v in given]
        for v in given:
            if np.iscomplexobj(v) or v.dtype.kind not in "fiub":
                msg = f"variance must hold real numbers, not {v.dtype}"
                raise TypeError(msg)
    if not many and given[0].ndim == 3:
        given = [given[0][i] for i in range(given[0].shape[0])]
        many = True
    if not many:
        given = given * len(frames)
    if len(given) != len(frames):
        msg = f"variance has {len(given)} entries for {len(frames)} frames"
        raise ValueError(msg)
    for v in given:
        if tuple(v.shape) != shape:
            msg = f"A variance frame of shape {tuple(v.shape)} does not fit frames of shape {shape}"
            raise IncorrectShapeError(msg)
    return given


def fit_stars_weighted(images, stars, psf, radius: float, mask=None, *, variance=None, sky_variance: float | None = None,
                       gain: float | None = None, background: str = "mesh", box: int = 64, fit_background: bool = True, cells=None,
                       device: int = 0) -> list[np.ndarray]:
    """``fit_stars`` with one weight per pixel, ``w = 1 / v``, and the formal errors of what it fits: a list of NumPy structured arrays
    (``weighted_fit_dtype``), one per frame and one row per position.  The dtype holds every field of ``fit_dtype`` by name, so
    ``cell_fit_summary``, ``subtract_stars``, ``build_subtracted`` and its ``keep=`` take the result as it is, and adds ``sw, swm, flux_err,
    background_err, flux_background_cov, snr, chi2_reduced``.

    ``images``, ``stars``, ``psf``, ``radius``, ``mask``, ``background``, ``box``, ``fit_background``, ``cells`` and ``device`` are
    ``fit_stars``'.  The variance ``v`` of a pixel comes from exactly one of two sources (anything else is a ``ValueError``):

    ``variance``: a map - one array of the frames' shape for all frames, or one per frame (a list, or a 3-D array).  Host arrays go with host
    frames; ``DeviceArray`` s, or objects with ``__cuda_array_interface__``, with the dtypes and strides ``apply`` takes, go with device
    frames; mixing the two is a ``TypeError``, a wrong shape an ``IncorrectShapeError``.  The map is rounded to float32 once, as a frame
    is, and ``v = (double) map[p]``.

    ``sky_variance`` (and ``gain``): the noise model ``v = sky_variance + max(pixel, 0) / gain`` on the raw float32 pixel, not on the
    background-subtracted one.  ``sky_variance >= 0`` and finite, ``gain > 0``; ``gain=None`` is ``+inf`` and drops the photon term, and
    then ``sky_variance`` must be positive.  ``gain`` is only allowed with ``sky_variance``.

    Kernel S12 (``rpsf_stars_fit_weighted``; DESIGN.md 3.7 "Weighted fits") is S8 with weights: the same box, disc ``q <= R^2``, model
    ``m``, residual ``d``, summation order and flags.  A pixel is usable when ``fit_stars``' rule holds (finite, unmasked, on the frame)
    and ``w = 1 / v`` is positive and finite: a ``v`` that is NaN, ``<= 0``, ``+inf`` or so small that ``w`` overflows takes the pixel out
    of the fit.  It still counts in ``n_all`` and ``sm_all`` and shows as lower ``coverage``; there is no flag of its own.  Over the usable
    pixels: ``n_use``, ``sm = sum m`` (unweighted, so ``coverage = sm / sm_all`` keeps its meaning), ``sw = sum w``, ``swm = sum w m``,
    and in the fields ``smm, sd, sdm, sdd`` the weighted sums ``sum w m^2, sum w d, sum w d m, sum w d^2``.  With ``fit_background``:
    ``D = sw smm - swm^2``, ``flux = (sw sdm - swm sd) / D``, ``background = (sd - flux swm) / sw``, ``var(flux) = sw / D``,
    ``var(background) = smm / D``, ``flux_background_cov = - swm / D``; without: ``D = smm``, ``flux = sdm / D``, ``background = 0``,
    ``var(flux) = 1 / D``, the other two 0.  Flags are ``fit_stars``' (``TOO_FEW`` on ``n_use``, ``DEGENERATE`` on ``D``); with any of
    them ``flux``, ``background``, the errors and the residual's columns are NaN.  With ``e = d - (flux m + background)``: ``chi2 = sum w
    e^2``; ``abs_res = sum |e|``, ``residual_fraction`` and the peak are unweighted, ``fit_stars``'.  Derived here in NumPy float64
    (``weighted_fit_from_sums``): ``flux_err = sqrt(var(flux))``, ``background_err``, ``snr = flux / flux_err``, ``dof = n_use - 2``
    (``- 1`` without a fitted background), ``chi2_reduced = chi2 / dof`` (NaN when ``dof <= 0``) and ``rms = sqrt(chi2_reduced)``.

    With ``v = 1`` everywhere ``flux``, ``background``, ``chi2``, ``abs_res`` and the peak are ``fit_stars``' bit for bit.  With ``v = 2^k``
    everywhere ``flux``, ``background``, ``abs_res`` and the peak stay, ``chi2`` is ``2^-k`` times ``fit_stars``' and ``var(flux)`` is
    ``2^k n / D`` of ``fit_stars``' sums, exactly.

    What this is NOT: positions are fixed, not fitted (``refine_stars`` and ``fit_positions`` supply them); the model is bilinear and cut at
    ``R``; the errors are formal - what the given variances imply for a linear fit, and nothing else: no model error, no position error, no
    correlation between pixels, and wrong variances give wrong errors; ``fit_positions`` and ``fit_groups`` stay unweighted.
    """
    if (variance is None) == (sky_variance is None):
        msg = "give the pixel variances either as a map (variance=) or as a noise model (sky_variance=, gain=), not both and not neither"
        raise ValueError(msg)
    if gain is not None and sky_variance is None:
        msg = "gain belongs to the noise model: it is only allowed with sky_variance"
        raise ValueError(msg)
    if sky_variance is not None:
        try:
            sky_variance, gain = float(sky_variance), np.inf if gain is None else float(gain)
        except (TypeError, ValueError) as error:
            msg = f"sky_variance and gain must be numbers, not {sky_variance!r} and {gain!r}"
            raise ValueError(msg) from error
        if not (sky_variance >= 0.0 and np.isfinite(sky_variance)):
            msg = f"sky_variance must be finite and not negative, got {sky_variance}"
            raise ValueError(msg)
        if not gain > 0.0:
            msg = f"gain must be positive (None or inf: no photon term), got {gain}"
            raise ValueError(msg)
        if sky_variance == 0.0 and np.isinf(gain):
            msg = "sky_variance = 0 without a gain leaves no variance at all"
            raise ValueError(msg)
    frames, masks, positions, cells, values, radius = _fit_inputs(images, stars, psf, radius, mask, background, box, fit_background, cells,
                                                                  device)
    variances = [None] * len(frames) if variance is None else _variance_frames(variance, frames, device)
    with _fit_session(frames, masks, positions, cells, values, box, device) as (finder, model, each_frame):
        out, last = [], None
        for k, p, c in each_frame:
            v = variances[k]
            if v is not None and v is not last:  # (one map for all frames goes up once)
                finder.variance(v)
                last = v
            rows = finder.fit_weighted(model, p, c, radius, bool(fit_background), background == "mesh", sky_variance,
                                       np.inf if gain is None else gain)
            out.append(weighted_fit_from_sums(rows, bool(fit_background)))
        return out


# ---------------------------------------------------------------------------------------------------------------------- fitted positions
FITPOS_FIELDS = ("row", "col", "row0", "col0", "niter", "flags", "converged", "step_row", "step_col", "ran_away", "not_converged", "singular",
                 "skipped", *("fit_flags" if name == "flags" else name for name in FIT_FIELDS if name not in ("row", "col")))


def fitpos_dtype() -> np.dtype:
    """The structured dtype of ``fit_positions``: the iteration's fields (``niter`` and ``flags`` int32, ``converged`` and the four booleans
    of the iteration's flags bool, the rest float64), then every field of ``fit_dtype`` but ``row`` and ``col``, ``fit_stars``' ``flags``
    under the name ``fit_flags``."""
    fit = fit_dtype()
    kinds = {"niter": np.int32, "flags": np.int32, "converged": np.bool_, "ran_away": np.bool_, "not_converged": np.bool_, "singular": np.bool_,
             "skipped": np.bool_, "fit_flags": fit["flags"], **{name: fit[name] for name in fit.names if name not in ("row", "col", "flags")}}
    return np.dtype([(name, kinds.get(name, np.float64)) for name in FITPOS_FIELDS])


def fitpos_from_sums(steps: np.ndarray, fits: np.ndarray, fit_background: bool = True) -> np.ndarray:
    """The structured result (``fitpos_dtype``) of S9's iteration rows and S8's rows at the positions they end at: ``converged = flags == 0
    and niter > 0``, one boolean per iteration flag, and ``fit_from_sums`` of the fit rows."""
    steps = np.asarray(steps, np.float64).reshape(-1, len(FITPOS_COLUMNS))
    col = {name: steps[:, j] for j, name in enumerate(FITPOS_COLUMNS)}
    fit = fit_from_sums(fits, fit_background)
    if len(fit) != len(steps):
        msg = f"{len(fit)} fit rows for {len(steps)} iteration rows"
        raise ValueError(msg)
    out = np.empty(len(steps), fitpos_dtype())
    for name in ("row", "col", "row0", "col0", "step_row", "step_col"):
        out[name] = col[name]
    out["niter"], out["flags"] = col["niter"].astype(np.int32), col["flags"].astype(np.int32)
    out["converged"] = (out["flags"] == 0) & (out["niter"] > 0)
    for name, bit in (("ran_away", FITPOS_RAN_AWAY), ("not_converged", FITPOS_NOT_CONVERGED), ("singular", FITPOS_SINGULAR),
                      ("skipped", FITPOS_SKIPPED)):
        out[name] = (out["flags"] & bit) != 0
    for name in fit.dtype.names:
        if name not in ("row", "col"):
            out["fit_flags" if name == "flags" else name] = fit[name]
    return out


def fit_positions(images, stars, psf, radius: float, mask=None, *, background: str = "mesh", box: int = 64, fit_background: bool = True,
                  cells=None, max_iter: int = 16, eps: float = 1e-4, max_shift: float = 2.0, max_step: float = 0.5,
                  device: int = 0) -> list[np.ndarray]:
    """Fit the position of every star with the cell of a PSF model it belongs to: a list of NumPy structured arrays (``fitpos_dtype``), one
    per frame and one row per star, with the fields ``row, col`` (the fitted position), ``row0, col0`` (the input), ``niter, flags,
    converged, step_row, step_col``, the booleans ``ran_away, not_converged, singular, skipped``, and then every field of ``fit_stars`` at
    the fitted position (``cell, flux, background, ..., residual_fraction, ...``; ``fit_stars``' flags are ``fit_flags``).  ``build(...,
    stars=fit_positions(...))``, ``star_photometry``, ``refine_stars`` and ``fit_stars`` take the result as it is.

    ``images``, ``stars``, ``psf``, ``radius``, ``mask``, ``background``, ``box``, ``fit_background`` and ``cells`` are ``fit_stars``'.  The
    cell of a star is chosen once, at the input position (``nearest_cells``), and stays for the whole iteration.  ``max_iter``: 0 ... 64; 0
    fits at the given positions.  ``eps > 0``: the iteration has converged when a step ``(dy, dx)`` has ``dy^2 + dx^2 < eps^2``.
    ``max_shift``: ``0 < max_shift <= 64``, the farthest a position may move from its start.  ``max_step``: ``0 < max_step <= 64``, the
    bound on either component of one step.

    One round at ``p = (row, col)``: over ``fit_stars``' pixels, with ``m`` the model and ``(g_u, g_v)`` the exact gradient of the bilinear
    interpolant there, the normal equations of ``d ~ f m + bg + a_u g_u + a_v g_v`` (without ``fit_background``: no ``bg``) are summed and
    solved by an LDL^T elimination without pivoting; the step is ``(-a_u / f, -a_v / f)``, each component clamped to ``max_step``.
    ``SKIPPED`` (8): the star has ``fit_stars``' ``NO_MESH`` or ``BAD_CELL``, nothing iterates.  ``SINGULAR`` (4): fewer usable pixels than
    unknowns, a pivot that is not finite or not positive (an all-zero, constant or NaN cell), or a step that is not finite; the star stays
    where it is.  ``RAN_AWAY`` (1): the step would end farther than ``max_shift`` from the start; it is rejected.  Otherwise the step is
    accepted; below ``eps`` the star has converged, after ``max_iter`` steps it is ``NOT_CONVERGED`` (2).  ``step_row, step_col`` are the
    last step taken or rejected (NaN if none), ``niter`` the steps accepted, ``converged`` is ``flags == 0 and niter > 0``.  The fit fields
    are kernel S8's at the position returned: ``fit_stars(frames, result, psf, radius, cells=[r["cell"] for r in result])`` gives the same
    bits.

    This is NOT a PSF-photometry package's fit: the weights are uniform - there is no error column and no variance weighting -, the
    interpolation is bilinear (the gradient is piecewise constant along its own axis, so the fitted position carries the model's sampling),
    the cell is fixed and not chosen again while the star moves, one star is fitted at a time - neighbours are not fitted together -, and
    masked pixels are excluded and reported through ``coverage``, not corrected for.
    """
    if isinstance(max_iter, (bool, np.bool_)) or not isinstance(max_iter, (int, np.integer)):
        msg = f"max_iter must be an integer, not {max_iter!r}"
        raise TypeError(msg)
    if not 0 <= max_iter <= MAX_ITER:
        msg = f"max_iter must lie in 0 ... {MAX_ITER}, got {max_iter}"
        raise ValueError(msg)
    if not (float(eps) > 0.0 and np.isfinite(eps)):
        msg = f"eps must be positive and finite, got {eps}"
        raise ValueError(msg)
    for name, value in (("max_shift", max_shift), ("max_step", max_step)):
        if not 0.0 < float(value) <= MAX_RADIUS:
            msg = f"{name} must lie in 0 < {name} <= {MAX_RADIUS:g}, got {value}"
            raise ValueError(msg)
    frames, masks, positions, cells, values, radius = _fit_inputs(images, stars, psf, radius, mask, background, box, fit_background, cells,
                                                                  device)
    with _fit_session(frames, masks, positions, cells, values, box, device) as (finder, model, each_frame):
        out = []
        for _, p, c in each_frame:
            steps, fits = finder.fit_positions(model, p, c, radius, bool(fit_background), int(max_iter), eps, max_shift, max_step,
                                               background == "mesh")
            out.append(fitpos_from_sums(steps, fits, bool(fit_background)))
        return out


# ---------------------------------------------------------------------------------------------------------------------- model and residual frames
def render_info() -> tuple[int, int, int]:
    """Kernel S10's tile (rows, columns) and the number of star records it stages at a time."""
    from regularizepsf_amd import _native

    rows, cols, chunk = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _native.check(_native.lib().rpsf_stars_render_info(ctypes.byref(rows), ctypes.byref(cols), ctypes.byref(chunk)))
    return rows.value, cols.value, chunk.value


def _check_render_out(out, shape: tuple[int, int], dtype: np.dtype, device: int | None = None) -> None:
    """``out=`` of one frame: a C-contiguous ``DeviceArray`` of the frame's shape and of ``dtype`` (on ``device`` when that is given)."""
    from regularizepsf_amd.device_array import DeviceArray

    if not isinstance(out, DeviceArray):
        msg = f"out takes one DeviceArray per frame, not {type(out).__name__}"
        raise TypeError(msg)
    if tuple(out.shape) != tuple(shape):
        msg = f"out has shape {out.shape}, the frame {tuple(shape)}"
        raise IncorrectShapeError(msg)
    if out.dtype != np.dtype(dtype):
        msg = f"out has dtype {out.dtype}, the call asks for {np.dtype(dtype)}"
        raise TypeError(msg)
    if not out.c_contiguous:
        msg = "out must be C-contiguous: the kernel writes dense rows"
        raise ValueError(msg)
    if device is not None and out.device != device:
        msg = f"out lives on device {out.device}, the call runs on device {device}"
        raise ValueError(msg)


def _render_outs(out, n_frames: int, shape: tuple[int, int], dtype: np.dtype, device: int) -> list:
    """``out=`` as one entry per frame (None: a host array is made), everything checked before anything runs."""
    if out is None:
        return [None] * n_frames
    outs = list(out) if isinstance(out, (list, tuple)) else [out]
    if len(outs) != n_frames:
        msg = f"out has {len(outs)} entries for {n_frames} frames"
        raise ValueError(msg)
    for o in outs:
        _check_render_out(o, shape, dtype, device)
    return outs


def _render_inputs(stars, n_frames: int | None, psf, radius, flux, cells, dtype) -> tuple:
    """What ``subtract_stars`` and ``render_stars`` make of their star arguments: ``(positions, fluxes, cells, values, radius, dtype)``,
    one entry per frame in the first three."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        msg = f"dtype must be float32 or float64, not {dtype}"
        raise TypeError(msg)
    coordinates, values = model_cube(psf)
    size = values.shape[1]
    try:
        radius = float(radius)
    except (TypeError, ValueError) as error:
        msg = f"radius must be a number, not {radius!r}"
        raise TypeError(msg) from error
    limit = min(MAX_RADIUS, size / 2 - 1)
    if not 0.0 < radius <= limit:
        msg = f"radius must lie in 0 < R <= min({MAX_RADIUS:g}, N / 2 - 1) = {limit:g} for cells of {size}, got {radius}"
        raise ValueError(msg)
    if isinstance(stars, np.ndarray) and (stars.dtype.names is not None or stars.ndim == 2):
        stars = [stars]  # one frame's stars, as they are
    stars = [np.asarray(s) for s in stars]
    if n_frames is not None and len(stars) != n_frames:
        msg = f"the stars have {len(stars)} entries for {n_frames} frames"
        raise ValueError(msg)
    positions = [np.ascontiguousarray(star_positions(s)) for s in stars]
    for i, p in enumerate(positions):
        if not np.all(np.abs(p) < MAX_COORD):  # (false for NaN)
            msg = f"stars[{i}] has a position that is not finite or not inside |row|, |col| < 2^20"
            raise ValueError(msg)

    def per_frame(given, name: str, kinds: str, kind_name: str, to) -> list:
        if isinstance(given, np.ndarray) and given.ndim == 1 and len(stars) == 1:
            given = [given]
        if len(given) != len(stars):
            msg = f"{name} has {len(given)} entries for {len(stars)} frames"
            raise ValueError(msg)
        result = []
        for i, (g, p) in enumerate(zip(given, positions)):
            g = np.asarray(g)
            if g.dtype.kind not in kinds and g.size:
                msg = f"{name}[{i}] must be {kind_name}, not {g.dtype}"
                raise TypeError(msg)
            if g.shape != (len(p),):
                msg = f"{name}[{i}] has shape {g.shape} for the {len(p)} stars of frame {i}"
                raise ValueError(msg)
            if to is np.int32 and g.size and (g.min() < -(2 ** 31) or g.max() >= 2 ** 31):
                msg = f"{name}[{i}] has an index outside int32"
                raise ValueError(msg)
            result.append(np.ascontiguousarray(g, to))
        return result

    if flux is None:
        if not all(s.dtype.names is not None and "flux" in s.dtype.names for s in stars):
            msg = "flux= is needed unless every entry of the stars is a structured array with a 'flux' field (fit_stars', fit_positions')"
            raise ValueError(msg)
        fluxes = [np.ascontiguousarray(s["flux"].ravel(), np.float64) for s in stars]
    else:
        fluxes = per_frame(flux, "flux", "fiu", "real numbers", np.float64)
    if cells is None:
        cells = [np.ascontiguousarray(s["cell"].ravel(), np.int32) if s.dtype.names is not None and "cell" in s.dtype.names
                 else nearest_cells(p, coordinates, size) for s, p in zip(stars, positions)]
    else:
        cells = per_frame(cells, "cells", "iu", "integers", np.int32)
    return positions, fluxes, cells, values, radius, dtype


def subtract_stars(images, fits, psf, radius: float, mask=None, *, flux=None, cells=None, background: str = "none", box: int = 64,
                   dtype=np.float32, out=None, return_model: bool = False, return_counts: bool = False, device: int = 0):
    """Take fitted stars out of their frames: a list of residual frames, one per frame, ``frame - sum of the stars``, every star drawn with
    its flux and its cell of the PSF model (kernel S10, DESIGN.md 3.7 "Model and residual frames").  It shows what ``cell_fit_summary``'s
    one number per cell cannot: wings, a ghost, a neighbour the model does not know.

    ``images`` are ``fit_stars``' images, device frames included.  ``fits``: the list ``fit_stars`` or ``fit_positions`` returns (one
    frame's array for one frame), taken by its fields ``row``, ``col``, ``flux`` and ``cell``; or anything ``star_positions`` accepts,
    together with ``flux=`` (one float array per frame).  ``cells=None`` uses the ``cell`` field when there is one, so that a star is
    drawn with the cell it was fitted with, and ``nearest_cells`` otherwise; or one integer array per frame.  ``psf`` and ``radius`` =
    ``R`` are ``fit_stars``': ``0 < R <= min(64, N / 2 - 1)``.  ``background``: ``"none"`` subtracts from the frame as it is, ``"mesh"``
    from the frame minus its background mesh of ``box`` (the ``d`` that ``fit_stars(background="mesh")`` fitted; a frame without a usable
    pixel is an error).  ``mask`` enters only through that mesh.  ``dtype``: float32 (the float64 result rounded once) or float64.
    ``out=``: one ``DeviceArray`` per frame (one for a single frame), C-contiguous, of the frame's shape and of ``dtype``, on ``device``;
    the kernel writes into it and it is returned in the list.  ``return_model=True`` also returns the model frames (host arrays of
    ``dtype``), ``return_counts=True`` also the number of stars drawn per frame: ``(residuals[, models][, counts])``.

    A star is drawn when its flux is finite and its cell is one of the model's; every other star is skipped, so the flagged rows of
    ``fit_stars``, whose flux is NaN, drop out by themselves.  At pixel ``(r, c)``: ``s = 0``; for the drawn stars in ascending index,
    when ``(r - row)^2 + (c - col)^2 <= R^2``: ``s += flux * m`` with ``m`` ``fit_stars``' model there, in float64; the residual is
    ``frame - s``.  NaN and Inf propagate as the arithmetic says; a pixel no star reaches comes back as its own bits.  Every pixel adds
    its stars in the same order on every run: two calls agree bit for bit.

    This is NOT a PSF-photometry package's subtraction: the interpolation is bilinear and does not conserve flux below the pixel scale,
    the disc cuts the model at ``R`` (wings beyond it stay in the residual, with a step at the disc's edge), and the constant that
    ``fit_stars(fit_background=True)`` fitted per star (``background``) is not subtracted.
    """
    if background not in ("mesh", "none"):
        msg = f'background must be "mesh" or "none", not {background!r}'
        raise ValueError(msg)
    if not MIN_BOX <= int(box) <= MAX_BOX:
        msg = f"box must lie in {MIN_BOX} ... {MAX_BOX}, got {box}"
        raise ValueError(msg)
    frames = _device_frames(images, device)
    if frames is None:
        frames = _frames(images)
    positions, fluxes, cells, values, radius, dtype = _render_inputs(fits, len(frames), psf, radius, flux, cells, dtype)
    shape = tuple(frames[0].shape)
    outs = _render_outs(out, len(frames), shape, dtype, device)
    masks = _masks(mask, frames)
    mode = RENDER_RESIDUAL_MESH if background == "mesh" else RENDER_RESIDUAL
    finder = _Finder(shape, box, device)
    model = None
    try:
        model = _Model(values, device)
        residuals, models, counts = [], [], []
        for frame, m, p, f, c, o in zip(frames, masks, positions, fluxes, cells, outs):
            finder.background_device(frame, m)
            residual, drawn = finder.render(model, p, f, c, radius, mode, dtype, o)
            residuals.append(residual)
            counts.append(drawn)
            if return_model:
                models.append(finder.render(model, p, f, c, radius, RENDER_MODEL, dtype)[0])
        result = (residuals, *((models,) if return_model else ()), *((counts,) if return_counts else ()))
        return result[0] if len(result) == 1 else result
    finally:
        if model is not None:
            model.close()
        finder.close()


def render_stars(shape, stars, flux, psf, radius: float, *, cells=None, dtype=np.float32, out=None, device: int = 0) -> list:
    """Model frames alone: a list with one frame of ``shape`` per entry of ``stars``, the sum of the entry's stars drawn on an empty
    frame with ``subtract_stars``' rule (kernel S10 in its model mode): frames synthesised from a PSF model.  ``stars``: what
    ``subtract_stars`` takes as ``fits`` (one array for one frame); ``flux``: one float array per entry, or None to take the ``flux``
    field; ``cells``, ``psf``, ``radius``, ``dtype`` and ``out=`` are ``subtract_stars``'.  A pixel that no star reaches is ``+0.0``.
    The same caveats hold: bilinear interpolation, the model cut at ``R``."""
    shape = tuple(int(n) for n in shape)
    if len(shape) != 2 or min(shape) <= 0:
        msg = f"shape must be (rows, columns), both positive, not {shape}"
        raise IncorrectShapeError(msg)
    positions, fluxes, cells, values, radius, dtype = _render_inputs(stars, None, psf, radius, flux, cells, dtype)
    outs = _render_outs(out, len(positions), shape, dtype, device)
    finder = _Finder(shape, 64, device)  # (the mesh is never computed: any box will do)
    model = None
    try:
        model = _Model(values, device)
        return [finder.render(model, p, f, c, radius, RENDER_MODEL, dtype, o)[0] for p, f, c, o in zip(positions, fluxes, cells, outs)]
    finally:
        if model is not None:
            model.close()
        finder.close()


CELL_FIT_DTYPE = np.dtype([("count", np.int64), ("residual_fraction", np.float64), ("relative_rms", np.float64), ("flux", np.float64)])


def cell_fit_summary(fits, psf) -> np.ndarray:
    """``fit_stars``' result folded into one row per cell of ``psf`` (in the order of ``psf.coordinates``; host NumPy only): ``count``, the
    number of stars of all frames fitted with the cell without a flag, and over those the medians of ``residual_fraction``, of ``rms /
    |flux|`` (``relative_rms``) and of ``flux``.  A cell without such a star has NaN everywhere except ``count``.  The map that shows where
    a model is bad.  ``fits``: the list ``fit_stars`` returns, or one frame's array."""
    n_cells = len(psf.coordinates)
    if isinstance(fits, np.ndarray):
        fits = [fits]
    def by_name(f) -> np.ndarray:  # fit_groups' rows have more fields than fit_dtype: taken by name
        f = np.asarray(f)
        if f.dtype.names is None or f.dtype == fit_dtype() or not set(FIT_FIELDS) <= set(f.dtype.names):
            return np.asarray(f, fit_dtype()).ravel()
        out = np.empty(f.size, fit_dtype())
        for name in FIT_FIELDS:
            out[name] = f[name].ravel()
        return out

    rows = np.concatenate([by_name(f) for f in fits]) if len(fits) else np.zeros(0, fit_dtype())
    rows = rows[(rows["flags"] == 0) & (rows["cell"] >= 0) & (rows["cell"] < n_cells)]
    out = np.zeros(n_cells, CELL_FIT_DTYPE)
    for name in ("residual_fraction", "relative_rms", "flux"):
        out[name] = np.nan
    order = np.argsort(rows["cell"], kind="stable")
    rows = rows[order]
    out["count"] = np.bincount(rows["cell"], minlength=n_cells)
    bounds = np.concatenate([[0], np.cumsum(out["count"])])
    with np.errstate(invalid="ignore", divide="ignore"):
        relative = rows["rms"] / np.abs(rows["flux"])
    for cell in np.flatnonzero(out["count"]):
        part = slice(bounds[cell], bounds[cell + 1])
        out["residual_fraction"][cell] = np.median(rows["residual_fraction"][part])
        out["relative_rms"][cell] = np.median(relative[part])
        out["flux"][cell] = np.median(rows["flux"][part])
    return out


# ---------------------------------------------------------------------------------------------------------------------- group fits
GROUP_FIT_FIELDS = (*FIT_FIELDS, "group", "group_size", "group_n", "group_dof", "group_chi2", "group_rms", "group_abs_res", "crowded")
GROUP_DTYPE = np.dtype([("group", np.int32), ("group_size", np.int32), ("crowded", np.bool_)])


def group_fit_dtype() -> np.dtype:
    """The structured dtype of ``fit_groups``: every field of ``fit_dtype``, then ``group``, ``group_size``, ``group_n`` and ``group_dof``
    (int32), ``group_chi2``, ``group_rms`` and ``group_abs_res`` (float64) and the boolean ``crowded``."""
    kinds = {name: fit_dtype()[name] for name in FIT_FIELDS}
    kinds.update({"group": np.int32, "group_size": np.int32, "group_n": np.int32, "group_dof": np.int32, "crowded": np.bool_})
    return np.dtype([(name, kinds.get(name, np.float64)) for name in GROUP_FIT_FIELDS])


def group_fit_from_sums(rows: np.ndarray, fit_background: bool = True, max_group: int = MAX_GROUP) -> np.ndarray:
    """The structured result (``group_fit_dtype``) of S11's rows: the fields of ``fit_from_sums`` on the first columns, unchanged, then
    ``crowded = group_size > max_group``, ``group_dof = group_n - p`` with ``p`` the unknowns of the fit the star was in (the members of
    a group fitted together, 1 for a star fitted alone, plus 1 with a fitted background) and ``group_rms = sqrt(group_chi2 / group_dof)``
    (NaN when ``group_dof <= 0``)."""
    rows = np.asarray(rows, np.float64).reshape(-1, len(GROUP_COLUMNS))
    single = fit_from_sums(rows[:, :len(FIT_COLUMNS)], fit_background)
    col = {name: rows[:, j] for j, name in enumerate(GROUP_COLUMNS)}
    out = np.empty(len(rows), group_fit_dtype())
    for name in FIT_FIELDS:
        out[name] = single[name]
    for name in ("group", "group_size", "group_n"):
        out[name] = col[name].astype(np.int32)
    out["crowded"] = out["group_size"] > int(max_group)
    members = np.where(out["crowded"], 1, out["group_size"])
    out["group_dof"] = out["group_n"] - (members + (1 if fit_background else 0))
    out["group_chi2"], out["group_abs_res"] = col["group_chi2"], col["group_abs_res"]
    with np.errstate(invalid="ignore", divide="ignore"):
        dof = out["group_dof"].astype(np.float64)
        out["group_rms"] = np.where(dof > 0, np.sqrt(col["group_chi2"] / np.where(dof > 0, dof, np.nan)), np.nan)
    return out


def fit_groups_info() -> tuple[int, int, int]:
    """The columns of a row of kernel S11, the largest group it fits, and the groups a workgroup takes."""
    from regularizepsf_amd import _native

    values = [ctypes.c_int(0) for _ in range(3)]
    _native.check(_native.lib().rpsf_stars_fit_groups_info(*(ctypes.byref(v) for v in values)))
    return tuple(v.value for v in values)


def _group_options(link, max_group, radius: float | None) -> tuple[float, int]:
    if isinstance(max_group, (bool, np.bool_)) or not isinstance(max_group, (int, np.integer)):
        msg = f"max_group must be an integer, not {max_group!r}"
        raise TypeError(msg)
    if not 1 <= int(max_group) <= MAX_GROUP:
        msg = f"max_group must lie in 1 ... {MAX_GROUP}, got {max_group}"
        raise ValueError(msg)
    if link is None and radius is not None:
        return 2.0 * radius, int(max_group)
    try:
        link = float(link)
    except (TypeError, ValueError) as error:
        msg = f"link must be a number, not {link!r}"
        raise TypeError(msg) from error
    if radius is None:
        if not (0.0 < link < np.inf):
            msg = f"link must be positive and finite, got {link}"
            raise ValueError(msg)
    elif not 0.0 < link <= 2.0 * radius:
        msg = f"link must lie in 0 < link <= 2 R = {2.0 * radius:g} (beyond it two discs share no pixel), got {link}"
        raise ValueError(msg)
    return link, int(max_group)


def star_groups(stars, link: float, *, max_group: int = MAX_GROUP, eligible=None) -> np.ndarray:
    """The grouping of ``fit_groups`` alone, on the host: a structured array (``group``, ``group_size``, ``crowded``) with one row per
    star of one frame.  Two stars are linked when ``(row_i - row_j)^2 + (col_i - col_j)^2 <= link^2`` in float64; the groups are the
    connected components; ``group`` is the smallest index of the star's component and ``group_size`` its size.  A component of more than
    ``max_group`` (``1 ... 8``) members is ``crowded``: ``fit_groups`` fits each of its members alone.  ``eligible``: None, or one boolean
    per star; a star that is not eligible links to nobody.  ``stars``: anything ``star_positions`` accepts."""
    from regularizepsf_amd import _native

    link, max_group = _group_options(link, max_group, None)
    positions = np.ascontiguousarray(star_positions(stars), np.float64).reshape(-1, 2)
    if not np.all(np.abs(positions) < MAX_COORD):
        msg = "stars has a position that is not finite or not inside |row|, |col| < 2^20"
        raise ValueError(msg)
    flags = None
    if eligible is not None:
        flags = np.ascontiguousarray(np.asarray(eligible, bool).ravel(), np.uint8)
        if len(flags) != len(positions):
            msg = f"eligible has {len(flags)} entries for {len(positions)} stars"
            raise ValueError(msg)
    labels, sizes, crowded = np.zeros(len(positions), np.int32), np.zeros(len(positions), np.int32), np.zeros(len(positions), np.uint8)
    _native.check(_native.lib().rpsf_stars_link_groups(len(positions), _native._ptr(positions), None if flags is None else _native._ptr(flags),
                                                       link, max_group, _native._ptr(labels), _native._ptr(sizes), _native._ptr(crowded)))
    out = np.empty(len(positions), GROUP_DTYPE)
    out["group"], out["group_size"], out["crowded"] = labels, sizes, crowded != 0
    return out


def fit_groups(images, stars, psf, radius: float, mask=None, *, background: str = "mesh", box: int = 64, fit_background: bool = True,
               cells=None, link: float | None = None, max_group: int = MAX_GROUP, device: int = 0) -> list[np.ndarray]:
    """``fit_stars`` with blended neighbours fitted together: a list of NumPy structured arrays (``group_fit_dtype``), one per frame and
    one row per position.  Stars whose fit discs overlap share pixels; fitted one at a time, each takes its neighbour's light as flux.
    Here the stars no further than ``link`` from one another (None: ``2 radius``, the distance at which two discs stop sharing pixels;
    ``0 < link <= 2 R``) form a group - the connected components of that graph, ``star_groups`` - and a group of ``2 ... max_group``
    members (``max_group`` in ``1 ... 8``; 1 fits every star alone) is fitted at once by linear least squares over the union of its
    discs: one flux per star and, with ``fit_background``, one constant for the group, the positions fixed (kernel S11,
    ``rpsf_stars_fit_groups``; DESIGN.md 3.7 "Group fits").  Every other argument is ``fit_stars``'.

    Every field of ``fit_dtype`` is there with its meaning: ``n_use, n_all, sm, sm_all, smm, sd, sdm, sdd`` and ``coverage`` are the
    star's own over its own disc, the bits ``fit_stars`` gives; ``flux`` is the star's flux of the joint fit and ``background`` the group's
    constant; ``chi2, abs_res, peak_res, peak_e, peak_row, peak_col`` are taken over the star's own disc from ``e = d - (sum of flux_b m_b +
    background)``, the sum over the members whose disc holds the pixel - what ``subtract_stars`` takes out there.  The per-star ``dof``
    stays ``fit_stars``' nominal ``n_use - 2`` (``- 1`` without a fitted background) and ``rms = sqrt(chi2 / dof)`` with it: neither
    counts the neighbours' parameters.  The group's own figures count every pixel of the union once: ``group`` (the smallest index of
    the group's stars), ``group_size``, ``group_n`` (its usable pixels), ``group_dof = group_n - p`` with ``p`` = members (+ 1 with a
    fitted background), ``group_chi2``, ``group_rms = sqrt(group_chi2 / group_dof)`` and ``group_abs_res``.  A star that is alone - no
    neighbour within ``link``, a cell index outside the model or a cell that is not all finite, a frame without a mesh, or ``crowded``: a
    component of more than ``max_group`` stars, which is broken up - is ``fit_stars``' row, bit for bit, and its group figures are its
    own.  ``TOO_FEW`` (``group_n < p``) and ``DEGENERATE`` (a pivot of the elimination not finite or ``<= 0``, or a flux that is not
    finite - an all-zero cell, two stars at one position) go to every member of a group and leave NaN in the fit's fields.

    This is NOT a PSF-photometry package's fit: the weights are uniform - there is no error column and no variance weighting -, the
    positions are fixed and not fitted (``fit_positions`` fits them, one star at a time), the interpolation is bilinear and does not
    conserve flux below the pixel scale, the model is cut at ``R``, the cell of a star is fixed, and masked pixels are excluded and
    reported through ``coverage``, not corrected for.  Near-coincident stars give a near-singular system and huge fluxes of opposite sign:
    nothing guards that but ``DEGENERATE`` at a non-positive pivot.
    """
    frames, masks, positions, cells, values, radius = _fit_inputs(images, stars, psf, radius, mask, background, box, fit_background, cells,
                                                                  device)
    link, max_group = _group_options(link, max_group, radius)
    with _fit_session(frames, masks, positions, cells, values, box, device) as (finder, model, each_frame):
        out = []
        for _, p, c in each_frame:
            rows = finder.fit_groups(model, p, c, radius, bool(fit_background), background == "mesh", link, max_group)
            out.append(group_fit_from_sums(rows, bool(fit_background), max_group))
        return out
