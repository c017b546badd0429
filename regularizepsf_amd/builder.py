"""Build a PSF model from star patches (API of regularizepsf/builder.py:128-265).

What the reference does per star in a Python loop (image_processing.py:95-121: slice the reflect-padded frame, spline-shift the
patch onto the pixel grid, subtract a background plane, test) and per lattice cell over Python lists (builder.py:53-102:
``np.nansum`` / ``np.nanmedian`` / ``np.nanpercentile``) runs in two HIP kernels behind ``rpsf_builder_*`` (include/rpsf.h).
The host keeps what is bookkeeping: the rounded corners and shift amounts (Python's half-to-even ``round``) and the cell
membership of every patch.  The final per-cell clean-up (builder.py:231-260) is ``clean_cell`` here, a few ``scipy.ndimage``
calls per cell, or with ``ArrayPSFBuilder(..., cleanup="device")`` a third kernel, which leaves to ``clean_cell`` only the cells whose
background fit it flags as degenerate.  ``interpolation_scale`` (image_processing.py:49-59, builder.py:225-235) is opt-in with
``ArrayPSFBuilder(..., interpolation="device")``: every frame is upscaled on the device (``scale_image`` is the same resampling as a
function of its own), the patches are cut at ``N * s`` pixels and every averaged cell is brought back to ``N x N`` by a block mean.
``psf_size`` goes from 4 to 256: up to 128 the patch of a star lives in LDS, from 129 on in a workspace in device memory that the native
handle owns (``rpsf_builder_create_wide``, DESIGN.md 3.6 "Wide sizes"); every route of ``build`` works at every size.

The boundary of the feature is the star list: ``build(..., stars=[...])`` takes the ``(row, col)`` positions ``sep.extract``
returns; without it ``sep`` is imported and called as the reference calls it - or, with ``ArrayPSFBuilder(..., finder="device")``,
this package's own detector (``regularizepsf_amd.stars``) finds them on the fused route of DESIGN.md 3.11: every frame is uploaded at
most once (not at all when it is a ``DeviceArray``), the stars are found and the patches cut from that one float32 frame on the device.

``build_subtracted`` is the rebuild of the loop build, fit, remove the neighbours, rebuild: every patch is cut with the fitted stars around
it taken out (kernel B1n, DESIGN.md 3.6 "Neighbour-subtracted patches"), everything after the patches is ``build``'s own code;
``build_iterative`` drives the loop.
"""

from __future__ import annotations

import ctypes
import pathlib
from collections.abc import Generator

import numpy as np

from regularizepsf_amd.exceptions import IncorrectShapeError, PSFBuilderError
from regularizepsf_amd.psf import ArrayPSF
from regularizepsf_amd.util import IndexedCube, calculate_covering

AVERAGE_METHODS = {"mean": 0, "median": 1, "percentile": 2}
REJECTED, ACCEPTED, DEGENERATE_RING = 0, 1, 2
CLEANED, DEGENERATE_CELL = 0, 1  # flags of a cell after the device clean-up
CLEANUPS = ("host", "device")
INTERPOLATIONS = ("off", "device")
FINDERS = ("sep", "device")
FINDER_OPTIONS = {"box": 64, "min_area": 5, "max_area": None,
                  "deblend": False, "deblend_contrast": 0.005, "deblend_prominence": 1.0}  # find_stars's defaults
REFINE_OPTIONS = {"refine_sigma": None}  # what finder_options takes besides: the window sigma of kernel S7 (stars.refine_stars), None = off
MAX_PATCH = 128  # the largest patch kernel B1 cuts: psf_size * interpolation_scale may not exceed it (psf_size alone goes to 256, B1w)


def _frames(images) -> list[np.ndarray]:
    """``_convert_to_generator`` (builder.py:17-43) as a list of 2-D frames.  A single 2-D array is one frame (the reference
    yields it forever)."""
    if isinstance(images, Generator):
        frames = list(images)
    elif isinstance(images, np.ndarray):
        if images.ndim == 3:
            frames = list(images)
        elif images.ndim == 2:
            frames = [images]
        else:
            msg = "Image data array must be 3D"
            raise IncorrectShapeError(msg)
    elif isinstance(images, list) and len(images) > 0 and isinstance(images[0], (str, pathlib.Path)):
        msg = "Reading frames from FITS files needs astropy, which this package does not depend on: load the arrays and pass them"
        raise NotImplementedError(msg)
    elif isinstance(images, list) and len(images) > 0 and all(isinstance(f, np.ndarray) for f in images):
        frames = images
    else:
        msg = "Unsupported type for `images`"
        raise TypeError(msg)
    for frame in frames:
        if not isinstance(frame, np.ndarray) or frame.ndim != 2:
            msg = "Every frame must be a two-dimensional array"
            raise IncorrectShapeError(msg)
    shape = None
    for frame in frames:  # the reference's message, builder.py:218-221
        if shape is None:
            shape = frame.shape
        elif shape != frame.shape:
            msg = ("Images must all be the same shape."
                   f"Found both {shape} and {frame.shape}.")
            raise PSFBuilderError(msg)
    if not frames:
        msg = "No frames to build a PSF model from"
        raise PSFBuilderError(msg)
    return frames


def _device_frames(images, device: int) -> list | None:
    """Frames that live on the GPU as a list of 2-D ``DeviceArray`` s on ``device`` - a 2-D or 3-D ``DeviceArray`` (or object with
    ``__cuda_array_interface__``) or a list of 2-D ones; None when ``images`` holds no device array at all (``_frames`` takes it then)."""
    from regularizepsf_amd.device_array import as_device_array, is_device_array

    if is_device_array(images):
        array = as_device_array(images, device, what="images")
        if array.ndim == 3:
            frames = [array[i] for i in range(array.shape[0])]
        elif array.ndim == 2:
            frames = [array]
        else:
            msg = "Image data array must be 3D"
            raise IncorrectShapeError(msg)
    elif isinstance(images, (list, tuple)) and any(is_device_array(f) for f in images):
        if not all(is_device_array(f) for f in images):
            msg = "`images` mixes host and device frames: pass all frames as NumPy arrays or all as device arrays"
            raise TypeError(msg)
        frames = [as_device_array(f, device, what="images") for f in images]
    else:
        return None
    shape = None
    for frame in frames:
        if frame.ndim != 2:
            msg = "Every frame must be a two-dimensional array"
            raise IncorrectShapeError(msg)
        if shape is None:
            shape = frame.shape
        elif shape != frame.shape:
            msg = ("Images must all be the same shape."
                   f"Found both {shape} and {frame.shape}.")
            raise PSFBuilderError(msg)
    if not frames or 0 in shape:
        msg = "No frames to build a PSF model from"
        raise PSFBuilderError(msg)
    return frames


def _dense_f32(frame):
    """A device frame as a dense float32 ``DeviceArray``: itself when it is one, else a copy through kernel C1 (``(float)(double)v`` for
    integers, the C cast for float64 - what the host route does to the same values)."""
    from regularizepsf_amd import _native
    from regularizepsf_amd.device_array import device_empty

    frame.synchronize()  # the builder's launches are on the null stream
    if frame.dtype == np.float32 and frame.c_contiguous and frame.ptr % 4 == 0:
        return frame
    dense = device_empty(frame.shape, np.float32, frame.device)
    _native.convert_view(frame._view2d(), dense._view2d(), frame.device)
    return dense


def _finder_options(finder: str, options) -> dict:
    """``finder_options`` of the constructor with find_stars's defaults and range checks."""
    from regularizepsf_amd.stars import MAX_BOX, MIN_BOX, deblend_options, refine_sigma_option

    if options is None:
        return {**FINDER_OPTIONS, **REFINE_OPTIONS}
    if finder != "device":
        msg = 'finder_options may only be given with finder="device"'
        raise ValueError(msg)
    if not isinstance(options, dict) or set(options) - set(FINDER_OPTIONS) - set(REFINE_OPTIONS):
        msg = f"finder_options is a dict with any of {(*FINDER_OPTIONS, *REFINE_OPTIONS)}, not {options!r}"
        raise ValueError(msg)
    merged = {**FINDER_OPTIONS, **REFINE_OPTIONS, **options}
    if not MIN_BOX <= int(merged["box"]) <= MAX_BOX:
        msg = f"box must lie in {MIN_BOX} ... {MAX_BOX}, got {merged['box']}"
        raise ValueError(msg)
    merged["deblend"], merged["deblend_contrast"], merged["deblend_prominence"] = deblend_options(
        merged["deblend"], merged["deblend_contrast"], merged["deblend_prominence"])
    merged["refine_sigma"] = refine_sigma_option(merged["refine_sigma"])
    return merged


def _find_stars(frame: np.ndarray, star_threshold: float, star_mask) -> np.ndarray:
    """image_processing.py:65-74 on the host (UNVERIFIED here: sep is not among this package's test dependencies)."""
    try:
        import sep
    except ImportError as error:
        msg = "Star finding needs the `sep` package; install it, or pass the star positions yourself with stars=[(k, 2) arrays of (row, col)]"
        raise ImportError(msg) from error
    background = sep.Background(frame)
    try:
        found = sep.extract(frame - background, star_threshold, err=background.globalrms, mask=star_mask)
    except Exception:  # noqa: BLE001  (the reference treats any failure as "no stars")
        return np.zeros((0, 2))
    return np.stack([np.asarray(found["y"], np.float64), np.asarray(found["x"], np.float64)], axis=-1)


def _scale(interpolation_scale) -> int:
    """``interpolation_scale`` as a Python int: an integer (of any integer type, or a float that is one) of at least 1."""
    try:
        scale = int(interpolation_scale)
        ok = scale == interpolation_scale and scale >= 1 and not isinstance(interpolation_scale, bool)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        msg = f"interpolation_scale must be an integer of at least 1, not {interpolation_scale!r}"
        raise ValueError(msg)
    return scale


def scaled_shape(shape: tuple[int, int], interpolation_scale: int) -> tuple[int, int]:
    """The shape ``_scale_image`` gives a frame (image_processing.py:53-58)."""
    return 1 + (shape[0] - 1) * interpolation_scale, 1 + (shape[1] - 1) * interpolation_scale


def _scale_frame(frame: np.ndarray, scale: int, device: int) -> np.ndarray:
    from regularizepsf_amd import _native as n

    if min(frame.shape) < 4:
        msg = f"interpolation_scale needs frames of at least 4 x 4 pixels (the cubic spline takes four points), not {frame.shape}"
        raise ValueError(msg)
    if frame.dtype != np.float32:
        frame = frame.astype(np.float64, copy=False)
    frame = np.ascontiguousarray(frame)
    out = np.empty(scaled_shape(frame.shape, scale), np.float64)
    n.check(n.lib().rpsf_scale_image(device, n._ptr(frame), int(frame.dtype == np.float64), frame.shape[0], frame.shape[1], scale, n._ptr(out)))
    return out


def scale_image(images, interpolation_scale: int, *, device: int = 0):
    """``_scale_image`` of the reference (image_processing.py:49-59) on the GPU: every frame resampled with the interpolating cubic
    spline ``RectBivariateSpline(arange(H), arange(W), frame)`` onto ``1 + (H - 1) s`` by ``1 + (W - 1) s`` samples, in float64.

    ``images`` is one 2-D frame, a 3-D stack or a list of frames; the result has the same form and is float64 (float32 frames are
    widened exactly, anything else is taken as float64).  ``find_stars(scale_image(frames, s))`` gives the ``stars=`` of
    ``ArrayPSFBuilder(..., interpolation="device").build(frames, interpolation_scale=s)``: positions in scaled-frame pixels.
    """
    scale = _scale(interpolation_scale)
    if _device_frames(images, device) is not None:
        msg = "scale_image takes host frames: resampling device frames is not supported, bring them to the host (to_host)"
        raise TypeError(msg)
    frames = _frames(images)
    out = [_scale_frame(frame, scale, device) for frame in frames]
    if isinstance(images, np.ndarray):
        return out[0] if images.ndim == 2 else np.stack(out)
    return out


def star_positions(stars) -> np.ndarray:
    """One frame's entry of ``build(..., stars=)`` as ``(k, 2)`` float64 ``(row, col)``: a plain array as it is, a structured array
    (``star_catalog``'s, whole or filtered) by its ``row`` and ``col`` fields."""
    stars = np.asarray(stars)
    if stars.dtype.names is None:
        return np.asarray(stars, np.float64).reshape(-1, 2)
    if "row" not in stars.dtype.names or "col" not in stars.dtype.names:
        msg = f"A structured star array needs the fields 'row' and 'col', not {stars.dtype.names}"
        raise ValueError(msg)
    return np.stack([stars["row"].astype(np.float64).ravel(), stars["col"].astype(np.float64).ravel()], axis=-1)


def star_geometry(positions: np.ndarray, psf_size: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Per star of one frame: the float corner ``position - N / 2`` that keys the patch (image_processing.py:76-79), the rounded
    corner (:96; ``np.rint`` rounds half to even exactly as Python's ``round``) and the shift amounts (:101)."""
    positions = np.asarray(positions, np.float64).reshape(-1, 2)
    corner = positions - psf_size / 2
    rounded = np.rint(corner)
    shift = -corner + rounded - 0.5
    return corner, rounded.astype(np.int64), shift


def cell_membership(patch_corners: np.ndarray, cell_corners: np.ndarray, psf_size: int) -> tuple[np.ndarray, np.ndarray]:
    """``_find_matches`` (builder.py:45-51) for every patch at once, as a CSR list: ``offsets`` (cells + 1, int64) and ``members``
    (int32 patch indices), cells in the order of ``cell_corners``, patches inside a cell in the order given.

    A patch belongs to a cell when its centre ``corner + N // 2`` lies in ``[cell, cell + N)`` on both axes.  The cells of a
    covering are the full product of their distinct rows and columns, so the rows and the columns are matched separately."""
    n_cells = len(cell_corners)
    centre = np.asarray(patch_corners, np.float64).reshape(-1, 2) + psf_size // 2
    rows, row_of = np.unique(cell_corners[:, 0], return_inverse=True)
    cols, col_of = np.unique(cell_corners[:, 1], return_inverse=True)
    table = np.full((len(rows), len(cols)), -1, np.int64)
    table[row_of, col_of] = np.arange(n_cells)
    pairs_cell, pairs_patch = [], []
    # lower <= centre < lower + N  <=>  lower in (centre - N, centre]
    r_lo, r_hi = np.searchsorted(rows, centre[:, 0] - psf_size, "right"), np.searchsorted(rows, centre[:, 0], "right")
    c_lo, c_hi = np.searchsorted(cols, centre[:, 1] - psf_size, "right"), np.searchsorted(cols, centre[:, 1], "right")
    patch_index = np.arange(len(centre))
    for dr in range(int((r_hi - r_lo).max(initial=0))):
        for dc in range(int((c_hi - c_lo).max(initial=0))):
            ok = (r_lo + dr < r_hi) & (c_lo + dc < c_hi)
            cells = table[(r_lo + dr)[ok], (c_lo + dc)[ok]]
            present = cells >= 0
            pairs_cell.append(cells[present])
            pairs_patch.append(patch_index[ok][present])
    cell = np.concatenate(pairs_cell) if pairs_cell else np.zeros(0, np.int64)
    patch = np.concatenate(pairs_patch) if pairs_patch else np.zeros(0, np.int64)
    order = np.lexsort((patch, cell))
    offsets = np.zeros(n_cells + 1, np.int64)
    np.cumsum(np.bincount(cell, minlength=n_cells), out=offsets[1:])
    return offsets, patch[order].astype(np.int32)


def background_plane(patch: np.ndarray) -> np.ndarray:
    """``calculate_background`` (image_processing.py:13-46) with the same SciPy calls, float64."""
    import scipy.linalg
    from scipy.ndimage import binary_dilation, binary_erosion

    rows, cols = np.indices(patch.shape)
    inner = binary_erosion(patch != 0)
    inner[0, :] = inner[-1, :] = False
    inner[:, 0] = inner[:, -1] = False
    ring = binary_dilation(inner) & ~inner
    ring &= patch < patch[patch.shape[1] // 2, patch.shape[0] // 2]
    design = np.c_[cols[ring], rows[ring], np.ones_like(cols[ring])]
    fit = scipy.linalg.lstsq(design, patch[ring])[0]
    plane = fit[0] * cols + fit[1] * rows + fit[2]
    plane[patch == 0] = np.nan
    return plane


def clean_cell(cell: np.ndarray) -> np.ndarray:
    """The per-cell clean-up of builder.py:238-258 on one averaged cell (float64; the input is not modified): second background
    fit, everything below 0.5 % of the centre dropped (eroded mask), the connected component of the centre kept and dilated
    by one pixel, unit sum."""
    from scipy.ndimage import binary_dilation, binary_erosion, label

    with np.errstate(invalid="ignore", divide="ignore"):
        patch = cell - background_plane(cell)
        patch[patch == 0] = np.nan
        centre = patch[patch.shape[0] // 2, patch.shape[1] // 2]
        patch[binary_erosion(patch < 0.005 * centre, border_value=1)] = np.nan
        patch[~np.isfinite(patch)] = 0
        labels = label(patch)[0]
        core = binary_dilation(labels == labels[labels.shape[0] // 2, labels.shape[1] // 2])
        patch = patch * core
        return patch / np.nansum(patch)


def model_on_device(stack, method: str, percentile: float, offsets: np.ndarray, members: np.ndarray) -> np.ndarray:
    """The cleaned cells of a filled stack with the averaging and the clean-up both on the device.  The kernel does not restate
    SciPy's minimum-norm fit for a cell whose ring has fewer than three pixels (or all on one line): it flags the cell and
    hands back its averaged values, and ``clean_cell`` does that one here - so the result is ``clean_cell``'s for every cell."""
    values, flags = stack.model(method, percentile, offsets, members)
    for c in np.flatnonzero(flags == DEGENERATE_CELL):
        values[c] = clean_cell(values[c])
    return values


class _Stack:
    """A native builder handle: the device stack of accepted float32 patches."""

    def __init__(self, psf_size: int, device: int, capacity: int, scale: int = 1) -> None:
        """``scale`` > 1: a scaled builder - ``add_frame`` takes the unscaled frame and upscales it on the device, the stack holds
        patches of ``patch_size = psf_size * scale``, the cells of ``average`` and ``model`` are ``psf_size`` wide."""
        from regularizepsf_amd import _native

        self._native, self.psf_size, self.scale = _native, int(psf_size), int(scale)
        self.patch_size = self.psf_size * self.scale
        self._handle = ctypes.c_void_p()
        if self.scale == 1 and self.psf_size > MAX_PATCH:  # the wide sizes, 129 ... 256 (anything above: the library's refusal)
            _native.check(_native.lib().rpsf_builder_create_wide(ctypes.byref(self._handle), device, self.psf_size, max(1, int(capacity))))
        elif self.scale == 1:
            _native.check(_native.lib().rpsf_builder_create(ctypes.byref(self._handle), device, self.psf_size, max(1, int(capacity))))
        else:
            _native.check(_native.lib().rpsf_builder_create_scaled(ctypes.byref(self._handle), device, self.psf_size, self.scale,
                                                                   max(1, int(capacity))))

    def add_frame(self, frame: np.ndarray, rounded: np.ndarray, shift: np.ndarray, saturation_threshold: float, star_minimum: float,
                  star_maximum: float) -> np.ndarray:
        n = self._native
        if frame.dtype != np.float32:
            frame = frame.astype(np.float64, copy=False)
        frame = np.ascontiguousarray(frame)
        corners = np.ascontiguousarray(rounded, np.int32).reshape(-1, 2)
        frac = np.ascontiguousarray(shift, np.float64).reshape(-1, 2)
        flags = np.zeros(len(corners), np.uint8)
        if self.scale == 1:
            n.check(n.lib().rpsf_builder_add_frame(self._handle, n._ptr(frame), int(frame.dtype == np.float64), frame.shape[0],
                                                   frame.shape[1], len(corners), n._ptr(corners), n._ptr(frac),
                                                   float(saturation_threshold), float(star_minimum), float(star_maximum), n._ptr(flags)))
        else:
            n.check(n.lib().rpsf_builder_add_frame_scaled(self._handle, n._ptr(frame), int(frame.dtype == np.float64), frame.shape[0],
                                                          frame.shape[1], self.scale, len(corners), n._ptr(corners), n._ptr(frac),
                                                          float(saturation_threshold), float(star_minimum), float(star_maximum),
                                                          n._ptr(flags)))
        return flags

    def add_frame_device(self, frame_ptr: int, shape: tuple[int, int], rounded: np.ndarray, shift: np.ndarray, saturation_threshold: float,
                         star_minimum: float, star_maximum: float) -> np.ndarray:
        """``add_frame`` on a dense float32 frame of ``shape`` at ``frame_ptr`` on the builder's device (a scaled builder: the scaled
        frame); nothing but the star list is uploaded."""
        n = self._native
        corners = np.ascontiguousarray(rounded, np.int32).reshape(-1, 2)
        frac = np.ascontiguousarray(shift, np.float64).reshape(-1, 2)
        flags = np.zeros(len(corners), np.uint8)
        n.check(n.lib().rpsf_builder_add_frame_device(self._handle, ctypes.c_void_p(frame_ptr), int(shape[0]), int(shape[1]), len(corners),
                                                      n._ptr(corners), n._ptr(frac), float(saturation_threshold), float(star_minimum),
                                                      float(star_maximum), n._ptr(flags)))
        return flags

    def add_frame_subtracted(self, frame, shape: tuple[int, int], model, positions: np.ndarray, flux: np.ndarray, cells: np.ndarray,
                             radius: float, own: np.ndarray, rounded: np.ndarray, shift: np.ndarray, saturation_threshold: float,
                             star_minimum: float, star_maximum: float) -> np.ndarray:
        """Kernel B1n: ``add_frame`` (``frame`` a host array) or ``add_frame_device`` (``frame`` the address of a dense float32 frame of
        ``shape`` on the builder's device) with the stars ``positions`` / ``flux`` / ``cells`` of ``model`` (a ``stars._Model``, None when
        there are no stars) taken out of every patch but the patch's own, ``own[k]`` (-1: nobody is left in)."""
        n = self._native
        corners = np.ascontiguousarray(rounded, np.int32).reshape(-1, 2)
        frac = np.ascontiguousarray(shift, np.float64).reshape(-1, 2)
        own = np.ascontiguousarray(own, np.int32).ravel()
        positions = np.ascontiguousarray(positions, np.float64).reshape(-1, 2)
        flux = np.ascontiguousarray(flux, np.float64).ravel()
        cells = np.ascontiguousarray(cells, np.int32).ravel()
        if len(own) != len(corners) or len(frac) != len(corners) or len(flux) != len(positions) or len(cells) != len(positions):
            msg = f"{len(own)} own indices and {len(frac)} shifts for {len(corners)} corners, {len(flux)} fluxes and {len(cells)} cells for {len(positions)} positions"
            raise ValueError(msg)
        flags = np.zeros(len(corners), np.uint8)
        handle = model._handle if len(positions) else None
        star_args = (handle, len(positions), n._ptr(positions), n._ptr(flux), n._ptr(cells), float(radius), len(corners), n._ptr(own),
                     n._ptr(corners), n._ptr(frac), float(saturation_threshold), float(star_minimum), float(star_maximum), n._ptr(flags))
        if isinstance(frame, np.ndarray):
            if frame.dtype != np.float32:
                frame = frame.astype(np.float64, copy=False)
            frame = np.ascontiguousarray(frame)
            n.check(n.lib().rpsf_builder_add_frame_subtracted(self._handle, n._ptr(frame), int(frame.dtype == np.float64), frame.shape[0],
                                                              frame.shape[1], *star_args))
        else:
            n.check(n.lib().rpsf_builder_add_frame_device_subtracted(self._handle, ctypes.c_void_p(frame), int(shape[0]), int(shape[1]),
                                                                     *star_args))
        return flags

    def load(self, patches: np.ndarray) -> None:
        p = np.ascontiguousarray(patches, np.float32).reshape(-1, self.patch_size, self.patch_size)
        self._native.check(self._native.lib().rpsf_builder_load_patches(self._handle, len(p), self._native._ptr(p)))

    def __len__(self) -> int:
        count = ctypes.c_size_t(0)
        self._native.check(self._native.lib().rpsf_builder_count(self._handle, ctypes.byref(count)))
        return count.value

    def patches(self, first: int = 0, count: int | None = None) -> np.ndarray:
        count = len(self) - first if count is None else count
        out = np.empty((count, self.patch_size, self.patch_size), np.float32)
        self._native.check(self._native.lib().rpsf_builder_patches(self._handle, first, count, self._native._ptr(out)))
        return out

    def average(self, method: str, percentile: float, offsets: np.ndarray, members: np.ndarray) -> np.ndarray:
        n = self._native
        offsets = np.ascontiguousarray(offsets, np.int64)
        members = np.ascontiguousarray(members, np.int32)
        cells = np.empty((len(offsets) - 1, self.psf_size, self.psf_size), np.float64)
        n.check(n.lib().rpsf_builder_average(self._handle, AVERAGE_METHODS[method], float(percentile), len(offsets) - 1, n._ptr(offsets),
                                             n._ptr(members), n._ptr(cells)))
        return cells

    def downscale(self, cells: np.ndarray) -> np.ndarray:
        """Kernel B4 alone on float64 cells of ``patch_size``: their block means, cells of ``psf_size``."""
        n = self._native
        cells = np.ascontiguousarray(cells, np.float64).reshape(-1, self.patch_size, self.patch_size)
        out = np.empty((len(cells), self.psf_size, self.psf_size), np.float64)
        n.check(n.lib().rpsf_builder_downscale(self._handle, len(cells), n._ptr(cells), n._ptr(out)))
        return out

    def clean(self, cells: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """Kernel B3 alone on float64 cells of the builder's size: (cleaned cells, flags).  A cell flagged DEGENERATE_CELL comes
        back as it went in."""
        n = self._native
        cells = np.ascontiguousarray(cells, np.float64).reshape(-1, self.psf_size, self.psf_size)
        out, flags = np.empty_like(cells), np.zeros(len(cells), np.uint8)
        n.check(n.lib().rpsf_builder_clean(self._handle, len(cells), n._ptr(cells), n._ptr(out), n._ptr(flags)))
        return out, flags

    def model(self, method: str, percentile: float, offsets: np.ndarray, members: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """``average`` then ``clean`` without the averaged cells leaving the device: (cleaned cells, flags).  A cell flagged
        DEGENERATE_CELL holds its averaged values."""
        n = self._native
        offsets = np.ascontiguousarray(offsets, np.int64)
        members = np.ascontiguousarray(members, np.int32)
        out = np.empty((len(offsets) - 1, self.psf_size, self.psf_size), np.float64)
        flags = np.zeros(len(offsets) - 1, np.uint8)
        n.check(n.lib().rpsf_builder_model(self._handle, AVERAGE_METHODS[method], float(percentile), len(offsets) - 1, n._ptr(offsets),
                                           n._ptr(members), n._ptr(out), n._ptr(flags)))
        return out, flags

    def clean_ms(self) -> float:
        """Device time of the last clean-up (B3) launch."""
        ms = ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_builder_clean_ms(self._handle, ctypes.byref(ms)))
        return ms.value

    def kernel_ms(self) -> tuple[float, float]:
        """Device time of the last patch (B1) and the last averaging (B2) launch."""
        b1, b2 = ctypes.c_double(0), ctypes.c_double(0)
        self._native.check(self._native.lib().rpsf_builder_kernel_ms(self._handle, ctypes.byref(b1), ctypes.byref(b2)))
        return b1.value, b2.value

    def close(self) -> None:
        if self._handle is not None and self._handle.value:
            self._native.lib().rpsf_builder_destroy(self._handle)
            self._handle = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def _first_of_equal_keys(corner: np.ndarray) -> np.ndarray:
    """Equal keys of one frame: ``dict.update`` keeps the first position and the last value - the same patch either way.  The indices of the
    first star of every distinct float corner, ascending."""
    _, first = np.unique(corner, axis=0, return_index=True)
    first.sort()
    return first


def _keep_accepted(keys: dict, frame_index: int, corner: np.ndarray, flags: np.ndarray, patch: int) -> None:
    """After the patch kernel of one frame: ``corner`` are the float corners of the patches it was given, ``flags`` its verdicts.  The
    accepted ones are keyed in their order; a degenerate ring is the caller's error."""
    if np.any(flags == DEGENERATE_RING):
        bad = corner[flags == DEGENERATE_RING][0] + patch / 2
        msg = (f"Frame {frame_index}: the patch of the star at {tuple(float(v) for v in bad)} has fewer than three border pixels below "
               "its centre (or all on one line), so no background plane can be fitted.")
        raise PSFBuilderError(msg)
    for row, col in corner[flags == ACCEPTED].tolist():
        keys[(frame_index, row, col)] = len(keys)


def _cells_of_stack(stack, keys: dict, shape: tuple[int, int], size: int, scale: int, average_method: str, percentile: float, cleanup: str,
                    return_patches: bool) -> tuple:
    """Everything ``build`` does with a filled stack while the handle lives: the covering, the membership, B2 (and B3 with
    ``cleanup="device"``) and the patches.  ``(corners, offsets, cells, patches)``; the cells are cleaned when ``cleanup == "device"``."""
    patch = size * scale
    if scale == 1:
        corners = calculate_covering(shape, size)
    else:  # builder.py:225-227 as it stands: the scaled shape times the scale
        scaled = scaled_shape(shape, scale)
        corners = calculate_covering((scaled[0] * scale, scaled[1] * scale), patch)
    offsets, members = cell_membership(np.array([k[1:] for k in keys], np.float64).reshape(-1, 2), corners, patch)
    method = "median" if (average_method == "percentile" and percentile == 50) else average_method
    if cleanup == "device":
        cells = model_on_device(stack, method, percentile, offsets, members)
    else:
        cells = stack.average(method, percentile, offsets, members)
    patches = None
    if return_patches:
        values = stack.patches().astype(np.float64)
        patches = {key: values[index] for key, index in keys.items()}
    return corners, offsets, cells, patches


def _build_result(corners, offsets, cells, patches, cleanup: str, return_patches: bool):
    """``build``'s return values from what ``_cells_of_stack`` left."""
    counts = {tuple(corner): int(offsets[c + 1] - offsets[c]) for c, corner in enumerate(corners)}
    coordinates = [(corner[0], corner[1]) for corner in corners]
    values = cells if cleanup == "device" else np.stack([clean_cell(cell) for cell in cells])
    psf = ArrayPSF(IndexedCube(coordinates, values))
    return (psf, counts, patches) if return_patches else (psf, counts)


def _keeps(keep, counts: list[int]) -> list[np.ndarray]:
    """``keep=`` of ``build_subtracted`` as one boolean array per frame (None: every row)."""
    if keep is None:
        return [np.ones(n, bool) for n in counts]
    if isinstance(keep, np.ndarray) and keep.ndim == 1 and len(counts) == 1:
        keep = [keep]
    if len(keep) != len(counts):
        msg = f"keep has {len(keep)} entries for {len(counts)} frames"
        raise ValueError(msg)
    result = []
    for i, (k, n) in enumerate(zip(keep, counts)):
        k = np.asarray(k)
        if k.dtype != np.bool_:
            msg = f"keep[{i}] must be booleans, not {k.dtype}"
            raise TypeError(msg)
        if k.shape != (n,):
            msg = f"keep[{i}] has shape {k.shape} for the {n} stars of frame {i}"
            raise ValueError(msg)
        result.append(k)
    return result


class ArrayPSFBuilder:
    """A builder that takes a series of images and constructs an ArrayPSF to represent their implicit PSF."""

    def __init__(self, psf_size: int, device: int = 0, *, finder: str = "sep", finder_options: dict | None = None,
                 interpolation: str = "off", cleanup: str = "host") -> None:
        """``interpolation`` says what ``build`` does with ``interpolation_scale != 1``: ``"off"`` refuses it, ``"device"`` upscales
        every frame on the GPU, cuts the patches at ``psf_size * interpolation_scale`` pixels and block-averages every cell back to
        ``psf_size`` before the clean-up, as the reference does.  With ``interpolation_scale == 1`` the two settings are the same build.

        ``cleanup`` says where ``build`` runs the per-cell clean-up: ``"host"`` is ``clean_cell`` on every cell, ``"device"`` the
        third kernel, with ``clean_cell`` only on the cells it flags (a degenerate background fit) - the same model within 1e-12.
        It is an argument of the builder and not of ``build``, whose parameter list stays the reference's plus ``stars``.

        ``finder`` says who finds the stars when ``build`` gets no ``stars``: ``"sep"`` imports ``sep`` as the reference does,
        ``"device"`` is this package's detector (``find_stars``; it is not ``sep``) on the fused route: per frame one upload at most, the
        background mesh filtered on the device, the patches cut from the frame the stars were found in - bit for bit
        ``build(frames, stars=find_stars(frames, star_threshold, sep_mask, **finder_options))``.  ``finder_options``: a dict with any of
        ``box``, ``min_area``, ``max_area``, ``deblend``, ``deblend_contrast``, ``deblend_prominence`` (``find_stars``'s defaults) and
        ``refine_sigma`` (default None), only with ``finder="device"``.  With ``refine_sigma = s`` the detections are moved to their
        Gaussian-windowed positions (kernel S7, ``refine_stars``' defaults, the finder's own background) on the finder's frame before
        the patches are cut; a detection whose iteration ends with ``NO_FLUX`` or ``RAN_AWAY`` keeps its position.  The build is then
        bit for bit ``build(frames, stars=[refined_positions(f, r) for f, r in zip(found, refine_stars(frames, found, s, sep_mask,
        box=box))])`` with ``found = find_stars(frames, star_threshold, sep_mask, ...)`` (``stars.refined_positions``)."""
        if finder not in FINDERS:
            msg = f"finder must be one of {FINDERS}, not {finder!r}"
            raise ValueError(msg)
        self._finder_options = _finder_options(finder, finder_options)
        self._refine_sigma = self._finder_options.pop("refine_sigma")  # S7's, kept apart from the detector's own options
        self._finder = finder
        self._found_stars: list[np.ndarray] | None = None
        if cleanup not in CLEANUPS:
            msg = f"cleanup must be one of {CLEANUPS}, not {cleanup!r}"
            raise ValueError(msg)
        if interpolation not in INTERPOLATIONS:
            msg = f"interpolation must be one of {INTERPOLATIONS}, not {interpolation!r}"
            raise ValueError(msg)
        self._interpolation = interpolation
        self._psf_size = psf_size
        self._device = device
        self._cleanup = cleanup

    @property
    def psf_size(self) -> int:
        return self._psf_size

    @property
    def cleanup(self) -> str:
        return self._cleanup

    @property
    def interpolation(self) -> str:
        return self._interpolation

    @property
    def finder(self) -> str:
        return self._finder

    @property
    def found_stars(self) -> list[np.ndarray] | None:
        """After a build that found the stars itself with ``finder="device"``: the ``(k, 2)`` float64 ``(row, col)`` arrays it used, one
        per frame, in scaled-frame pixels when ``interpolation_scale > 1``.  None before a build and after a build with ``stars=``."""
        return self._found_stars

    def build(self, images, sep_mask=None, hdu_choice: int | None = 0, num_workers: int | None = None,  # noqa: ARG002
              interpolation_scale: int = 1, star_threshold: int = 3, average_method: str = "median", percentile: float = 50,
              saturation_threshold: float = np.inf, image_mask: np.ndarray | None = None, star_minimum: float = 0,
              star_maximum: float = np.inf, sqrt_compressed: bool = False, return_patches: bool = False, *,
              stars: list[np.ndarray] | None = None):
        """Build the PSF model: ``(ArrayPSF, counts)`` or, with ``return_patches``, ``(ArrayPSF, counts, patches)``.

        Parameters, their order and their defaults are the reference's (builder.py:139-153); ``num_workers`` is accepted and
        ignored (the patches are cut on the GPU).  ``stars`` is this package's addition: one ``(k, 2)`` float array of
        ``(row, col)`` star positions per frame - the ``y``, ``x`` columns of ``sep.extract`` - which skips star finding; a structured
        array with ``row`` and ``col`` fields, as ``star_catalog`` returns per frame (whole or filtered, e.g.
        ``cat[cat["elongation"] < 1.5]``), is taken by those two fields.
        ``patches`` maps ``(frame, row - N / 2, col - N / 2)`` to the float64 copy of the float32 patch kept on the device
        (background-subtracted, not normalised); ``counts`` maps every corner of the covering to its number of stars.

        ``images`` may also live on the builder's device: a 2-D or 3-D ``DeviceArray`` or a list of 2-D ``DeviceArray`` s / objects with
        ``__cuda_array_interface__`` (dtypes and strides as for ``apply``; ``interpolation_scale`` must be 1).  They are read where they
        lie and give what the host call gives on the same values.  ``sep_mask`` is always a host array.

        Without ``stars`` and with ``ArrayPSFBuilder(..., finder="device")`` the stars are found on the device, with ``star_threshold`` in
        units of the global background rms and ``sep_mask`` as ``find_stars``'s mask (one 2-D boolean array or one per frame, True =
        ignore); ``found_stars`` holds them afterwards.

        ``interpolation_scale = s > 1`` needs ``ArrayPSFBuilder(..., interpolation="device")``.  Then ``stars`` are positions in the
        SCALED frame (what ``sep.extract`` returns on it: ``find_stars(scale_image(frames, s))``), the patches are ``N s`` wide with
        keys ``(frame, row - N s / 2, col - N s / 2)``, and the covering is the reference's: cells of ``N s`` pixels over
        ``(Hs s, Ws s)`` with ``Hs = 1 + (H - 1) s`` (builder.py:225 multiplies the shape that is already scaled once more).
        """
        size = self._psf_size
        scale = _scale(interpolation_scale)
        if scale != 1 and self._interpolation == "off":
            msg = ('interpolation_scale != 1 is opt-in: construct the builder with ArrayPSFBuilder(..., interpolation="device") to resample '
                   "the frames on the GPU")
            raise NotImplementedError(msg)
        patch = size * scale  # the size patches are cut, shifted and averaged at
        if scale != 1 and patch > MAX_PATCH:
            msg = f"psf_size * interpolation_scale = {patch} is not implemented: the patch kernels stop at {MAX_PATCH} pixels"
            raise NotImplementedError(msg)
        if image_mask is not None:
            msg = "image_mask is not implemented (the reference spline-shifts the boolean mask; what that yields is defined by SciPy's cast only)"
            raise NotImplementedError(msg)
        if sqrt_compressed:
            msg = "sqrt_compressed=True is not implemented (the decompression scale comes from a FITS header)"
            raise NotImplementedError(msg)
        if average_method not in AVERAGE_METHODS:
            msg = f"Unknown method {average_method}."
            raise PSFBuilderError(msg)
        cleanup = self._cleanup
        self._found_stars = None
        frames = _device_frames(images, self._device)
        on_device = frames is not None
        if on_device and scale != 1:
            msg = "interpolation_scale != 1 takes host frames: resampling device frames is not supported, bring them to the host (to_host)"
            raise TypeError(msg)
        if not on_device:
            frames = _frames(images)
        if scale != 1 and min(frames[0].shape) < 4:
            msg = f"interpolation_scale needs frames of at least 4 x 4 pixels (the cubic spline takes four points), not {frames[0].shape}"
            raise ValueError(msg)
        seen_shape = tuple(frames[0].shape) if scale == 1 else scaled_shape(frames[0].shape, scale)  # of the frame the patches are cut from
        fused = stars is None and self._finder == "device"
        finder = None
        if fused:
            from regularizepsf_amd import stars as star_finder

            options = self._finder_options
            masks = star_finder._masks(sep_mask, frames, seen_shape)
            finder = star_finder._Finder(seen_shape, options["box"], self._device)
            if options["deblend"]:
                finder.set_deblend(True, options["deblend_contrast"], options["deblend_prominence"])
            stars = [None] * len(frames)
        elif stars is None:
            if on_device:
                msg = 'Star finding with `sep` takes host frames: construct the builder with ArrayPSFBuilder(..., finder="device") or pass stars='
                raise TypeError(msg)
            masks = [None] * len(frames) if sep_mask is None else _frames(sep_mask)
            seen = frames if scale == 1 else [_scale_frame(frame, scale, self._device) for frame in frames]  # sep sees the scaled frame
            stars = [_find_stars(frame, star_threshold, mask) for frame, mask in zip(seen, masks)]
        elif len(stars) != len(frames):
            msg = f"stars has {len(stars)} entries for {len(frames)} frames"
            raise ValueError(msg)
        else:
            stars = [star_positions(s) for s in stars]

        capacity = 1 if fused else sum(len(np.asarray(s).reshape(-1, 2)) for s in stars)  # (the stack grows by itself)
        stack = None
        try:
            stack = _Stack(size, self._device, capacity) if scale == 1 else _Stack(size, self._device, capacity, scale)
            found: list[np.ndarray] = []
            keys: dict[tuple[int, float, float], int] = {}  # patch key -> index into the device stack, in insertion order
            for i, (frame, positions) in enumerate(zip(frames, stars)):
                if fused:  # S1, S1b, S2 - S4 on the one device copy of the frame; B1 below cuts from the same
                    if scale == 1:
                        finder.background_device(frame, masks[i])
                    else:
                        finder.background_scaled(frame, scale, masks[i])
                    rows = finder.detect_device(float(star_threshold), int(options["min_area"]), options["max_area"])
                    positions = np.ascontiguousarray(rows[:, :2])
                    if self._refine_sigma is not None:  # S7 on the same frame and mesh; the star list crosses once more
                        positions = star_finder.refine_detections(finder, positions, self._refine_sigma)
                    found.append(positions)
                corner, rounded, shift = star_geometry(positions, patch)
                first = _first_of_equal_keys(corner)
                if fused:
                    flags = stack.add_frame_device(finder.frame_ptr(), seen_shape, rounded[first], shift[first], saturation_threshold,
                                                   star_minimum, star_maximum) if len(first) else np.zeros(0, np.uint8)
                elif on_device:
                    dense = _dense_f32(frame)  # (kept alive until B1 has run: add_frame_device waits for it)
                    flags = stack.add_frame_device(dense.ptr, seen_shape, rounded[first], shift[first], saturation_threshold, star_minimum,
                                                   star_maximum)
                else:
                    flags = stack.add_frame(frame, rounded[first], shift[first], saturation_threshold, star_minimum, star_maximum)
                _keep_accepted(keys, i, corner[first], flags, patch)
            corners, offsets, cells, patches = _cells_of_stack(stack, keys, tuple(frames[0].shape), size, scale, average_method, percentile,
                                                               cleanup, return_patches)
        finally:
            if stack is not None:
                stack.close()
            if finder is not None:
                finder.close()
        if fused:
            self._found_stars = found
        return _build_result(corners, offsets, cells, patches, cleanup, return_patches)

    def build_subtracted(self, images, fits, psf, radius: float, *, flux=None, cells=None, keep=None, average_method: str = "median",
                         percentile: float = 50, saturation_threshold: float = np.inf, star_minimum: float = 0,
                         star_maximum: float = np.inf, return_patches: bool = False):
        """``build(images, stars=...)`` with the fitted neighbours of every star taken out of its patch (kernel B1n, DESIGN.md 3.6
        "Neighbour-subtracted patches"): the rebuild of the loop build, fit, remove the neighbours, rebuild.  The return values are
        ``build``'s.

        ``fits``, ``psf``, ``radius``, ``flux`` and ``cells`` are ``subtract_stars``': per frame what ``fit_stars`` / ``fit_positions`` /
        ``fit_groups`` return, taken by ``row, col, flux, cell`` - flagged rows, whose flux is NaN, drop out of the subtraction set by
        themselves - or plain positions with ``flux=`` (and optionally ``cells=``).  ``psf`` is the model the stars are drawn with
        (its cells need not be ``psf_size`` wide), ``0 < radius <= min(64, N_m / 2 - 1)`` the disc a star is drawn in.  ``keep``: one
        boolean array per frame (one array for a single frame) saying which rows are CUT as patches; every drawn row is still subtracted
        as a neighbour, so ``keep=[f["residual_fraction"] < 0.1 for f in fits]`` drops the stars that fit their cell badly.  A row that
        is cut but not drawn is cut with every drawn star taken out.

        The patch of row ``i`` is, bit for bit, the patch ``build`` cuts at that position from the float32 frame
        ``subtract_stars(frame, fits, psf, radius)`` gives with the flux of row ``i`` set to NaN; where no drawn star's disc reaches
        another star's patch the result is ``build(images, stars=positions)``.  Everything after the patches - the keys and the
        first-of-equal-keys rule, the covering, the averaging, the clean-up according to ``cleanup=`` - is ``build``'s own code.  Host
        frames and device frames as in ``build``.  The caveats of ``subtract_stars`` hold: bilinear interpolation, the model cut at
        ``radius``, no per-star background.  ``psf_size`` above 128 and ``interpolation_scale`` are not implemented
        (``NotImplementedError``); a ``psf`` whose samples live on another device than the builder is a ``ValueError``."""
        from regularizepsf_amd import stars as star_module

        size = self._psf_size
        if size > MAX_PATCH:
            msg = f"psf_size = {size} is not implemented for neighbour-subtracted patches: kernel B1n stops at {MAX_PATCH} pixels"
            raise NotImplementedError(msg)
        if average_method not in AVERAGE_METHODS:
            msg = f"Unknown method {average_method}."
            raise PSFBuilderError(msg)
        held = getattr(psf, "_fft_dev", None)
        if held is not None and held[1] != self._device:
            msg = f"psf lives on device {held[1]}, the builder on device {self._device}"
            raise ValueError(msg)
        cleanup = self._cleanup
        frames = _device_frames(images, self._device)
        on_device = frames is not None
        if not on_device:
            frames = _frames(images)
        shape = tuple(frames[0].shape)
        positions, fluxes, cells, values, radius, _ = star_module._render_inputs(fits, len(frames), psf, radius, flux, cells, np.float32)
        keeps = _keeps(keep, [len(p) for p in positions])
        self._found_stars = None
        stack = model = None
        try:
            stack = _Stack(size, self._device, sum(int(k.sum()) for k in keeps))
            model = star_module._Model(values, self._device)
            keys: dict[tuple[int, float, float], int] = {}
            for i, (frame, p, f, c, k) in enumerate(zip(frames, positions, fluxes, cells, keeps)):
                own = np.flatnonzero(k)
                corner, rounded, shift = star_geometry(p[own], size)
                first = _first_of_equal_keys(corner)
                dense = _dense_f32(frame) if on_device else None  # (kept alive until B1n has run)
                flags = stack.add_frame_subtracted(dense.ptr if on_device else frame, shape, model, p, f, c, radius, own[first],
                                                   rounded[first], shift[first], saturation_threshold, star_minimum, star_maximum)
                _keep_accepted(keys, i, corner[first], flags, size)
            corners, offsets, averaged, patches = _cells_of_stack(stack, keys, shape, size, 1, average_method, percentile, cleanup,
                                                                  return_patches)
        finally:
            if stack is not None:
                stack.close()
            if model is not None:
                model.close()
        return _build_result(corners, offsets, averaged, patches, cleanup, return_patches)

    def build_iterative(self, images, stars, radius: float, *, iterations: int = 2, fit: str = "groups", keep=None, **build_keywords):
        """The loop build, fit, remove the neighbours, rebuild: ``psf = build(images, stars=stars)``, then ``iterations`` times ``fits =
        fit_groups(images, stars, psf, radius)`` (``fit="groups"``; ``fit_stars`` for ``fit="stars"``) and ``psf = build_subtracted(images,
        fits, psf, radius, keep=...)``.  ``(psf, counts, fits)`` of the last round.  ``keep``: None, what ``build_subtracted`` takes, or a
        callable that makes it from the round's ``fits``.  ``build_keywords``: ``average_method``, ``percentile``,
        ``saturation_threshold``, ``star_minimum`` and ``star_maximum``, given to every build; ``interpolation_scale`` is ``build``'s
        keyword and is refused here as ``build`` refuses what it does not implement (``NotImplementedError``), whatever its value.  A driver over the public calls and
        nothing else: the fits run with their defaults on the builder's device."""
        from regularizepsf_amd import stars as star_module

        if fit not in ("groups", "stars"):
            msg = f'fit must be "groups" or "stars", not {fit!r}'
            raise ValueError(msg)
        if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or iterations < 1:
            msg = f"iterations must be an integer of at least 1, not {iterations!r}"
            raise ValueError(msg)
        if "interpolation_scale" in build_keywords:
            msg = "interpolation_scale is not implemented for neighbour-subtracted patches: the patches are cut from the frames as they are"
            raise NotImplementedError(msg)
        allowed = ("average_method", "percentile", "saturation_threshold", "star_minimum", "star_maximum")
        if set(build_keywords) - set(allowed):
            msg = f"build_iterative takes the build keywords {allowed}, not {sorted(set(build_keywords) - set(allowed))}"
            raise TypeError(msg)
        if self._psf_size > MAX_PATCH:
            msg = f"psf_size = {self._psf_size} is not implemented for neighbour-subtracted patches: kernel B1n stops at {MAX_PATCH} pixels"
            raise NotImplementedError(msg)
        fitter = star_module.fit_groups if fit == "groups" else star_module.fit_stars
        psf, counts = self.build(images, stars=stars, **build_keywords)
        fits = None
        for _ in range(int(iterations)):
            fits = fitter(images, stars, psf, radius, device=self._device)
            psf, counts = self.build_subtracted(images, fits, psf, radius, keep=keep(fits) if callable(keep) else keep, **build_keywords)
        return psf, counts, fits


def build_subtracted(images, fits, psf, radius: float, *, psf_size: int | None = None, device: int = 0, cleanup: str = "host", **keywords):
    """``ArrayPSFBuilder(psf_size, device, cleanup=cleanup).build_subtracted(images, fits, psf, radius, **keywords)`` as a function;
    ``psf_size=None`` cuts the patches at the size of the model's cells."""
    from regularizepsf_amd.stars import model_cube

    size = model_cube(psf)[1].shape[1] if psf_size is None else psf_size
    return ArrayPSFBuilder(size, device, cleanup=cleanup).build_subtracted(images, fits, psf, radius, **keywords)


def build_iterative(images, stars, radius: float, *, psf_size: int, device: int = 0, cleanup: str = "host", **keywords):
    """``ArrayPSFBuilder(psf_size, device, cleanup=cleanup).build_iterative(images, stars, radius, **keywords)`` as a function."""
    return ArrayPSFBuilder(psf_size, device, cleanup=cleanup).build_iterative(images, stars, radius, **keywords)
