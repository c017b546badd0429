"""PSF-to-PSF transform applied patch-wise in the Fourier domain (API of regularizepsf/transform.py:25-177,284-289).

``construct`` evaluates the regularized transfer kernel with the K2 HIP kernel and ``apply`` runs the
fused K1 patch kernel; both go through the C ABI of include/rpsf.h.  There is no CPU fallback.
Differences from the reference that a caller can observe are listed in INTEGRATION.md (float32
arithmetic inside the kernels; patch sizes other than 16..256 powers of two run a hipFFT-based fallback).
"""

from __future__ import annotations

import hashlib
import math
import numbers
import pathlib
import threading
import weakref

import numpy as np

from regularizepsf_amd import _native, device_array
from regularizepsf_amd.exceptions import InvalidCoordinateError
from regularizepsf_amd.util import IndexedCube


def _kernel_stamp(cube: IndexedCube) -> tuple:
    """What the device copy of a transfer kernel was made from: identity, edit count and a fingerprint of the values.

    The reference multiplies by ``values`` as they are at every ``apply`` (transform.py:164), and ``IndexedCube`` does not
    copy them, so a caller may edit the array in place between two applies.  ``__setitem__`` is counted exactly; edits that
    bypass it (``cube.values[i] = ...``, ``k *= 2``) cannot go unnoticed since round 6: the array is made READ-ONLY while a device copy
    of it exists (``ArrayPSFTransform._freeze``), so such a write raises NumPy's ``ValueError: assignment destination is read-only``
    instead of being silently missed; ``with transform.edit() as k:``, ``cube[coordinate] = patch`` and ``transform.invalidate()``
    are the ways to edit.  The fingerprint below stays as the backstop for memory that is reachable through another, still writeable
    array (a view taken before the upload, a base array): one 64-byte line of every patch (at most 4096 patches, evenly spaced beyond
    that; the line's position inside the patch varies from patch to patch) - 20 ... 60 us, where the evenly strided 64 K-element sample
    of rounds 2-4 cost 0.3 ... 1.4 ms of cache misses per apply, more than a small frame's whole correction.
    """
    if getattr(cube, "_loader", None) is not None:  # still on the GPU only (construct from device-resident spectra): nobody can have edited it
        return ("deferred", id(cube), cube._edits)
    values = cube.values
    if values.ndim == 3 and values.flags.c_contiguous and values.itemsize in (8, 16) and values.size:
        words = values.reshape(-1).view(np.uint64)  # 1 (complex64) or 2 (complex128) words per element
        key = (values.shape, values.itemsize)
        cached = getattr(cube, "_stamp_index", None)
        if cached is None or cached[0] != key:  # (the sample's positions depend on the shape only: built once per cube, 10 us of every apply otherwise)
            wpp = values.shape[1] * values.shape[2] * (values.itemsize // 8)
            patches = np.arange(0, values.shape[0], max(1, values.shape[0] // 4096), dtype=np.int64)
            line = min(8, wpp)
            offset = (patches * 104729) % max(1, wpp - line + 1)
            cached = (key, ((patches * wpp + offset)[:, None] + np.arange(line, dtype=np.int64)[None, :]).reshape(-1))
            cube._stamp_index = cached
        sample = words[cached[1]]
        # (two wrap-around reductions of the sampled words instead of a cryptographic digest of their bytes: any change of one word changes both)
        return (id(values), cube._edits, values.shape, values.dtype.str, int(np.bitwise_xor.reduce(sample)), int(np.add.reduce(sample)))
    elif values.flags.c_contiguous or values.flags.f_contiguous:
        flat = values.reshape(-1, order="A")
        sample = flat[:: max(1, flat.size // 4096)]
    else:  # strided views are rare and small: hash everything
        sample = np.ascontiguousarray(values)
    digest = hashlib.blake2b(sample.tobytes(), digest_size=8).digest()
    return (id(values), cube._edits, values.shape, values.dtype.str, digest)


_INDEX_MAP_MODES = ("symmetric", "reflect", "edge", "wrap")  # np.pad modes that copy pixels: a mask follows the image through them


def _check_masks(mask, shape, frames: int | None, device: int, frames_on_device: bool):
    """The ``mask=`` argument of apply (``frames`` None: one 2-D mask) or apply_batch (one 2-D mask for all frames, or ``frames`` of them as a
    3-D stack or a sequence) as ``(on_device, [masks])`` with one mask or one per frame: host masks as bool arrays, device masks as uint8
    ``DeviceArray`` views.  Raises before anything runs: ``TypeError`` for a device mask with host frames, ``ValueError`` for a wrong
    shape, a wrong count or a device mask that is not uint8.  Touches no GPU."""
    if mask is None:
        return False, None
    shape = tuple(shape)
    if not device_array.is_device_array(mask) and not isinstance(mask, np.ndarray) and isinstance(mask, (list, tuple)):
        kinds = {device_array.is_device_array(m) for m in mask}
        if len(kinds) == 2:
            msg = "mask mixes host and device arrays"
            raise ValueError(msg)
        on_device = kinds == {True}
        items = list(mask) if on_device else None
    else:
        on_device, items = device_array.is_device_array(mask), None
    if on_device and not frames_on_device:
        msg = "a device mask goes with device frames; pass a NumPy mask with NumPy frames"
        raise TypeError(msg)
    if on_device:
        if items is None:
            stack = device_array.as_device_array(mask, device, what="mask")
            items = [stack] if stack.ndim == 2 else [stack[i] for i in range(stack.shape[0])] if stack.ndim == 3 and frames is not None else None
            if items is None:
                msg = f"mask must have the frame's shape {shape}, got {stack.shape}"
                raise ValueError(msg)
        else:
            items = [device_array.as_device_array(m, device, what="mask") for m in items]
        for m in items:
            if m.dtype != np.uint8:
                msg = f"a device mask must be uint8, got {m.dtype}"
                raise ValueError(msg)
            if any(s <= 0 for s, n in zip(m.strides, m.shape) if n > 1):
                msg = "a device mask needs positive strides"
                raise ValueError(msg)
    else:
        host = np.asarray(mask)
        if host.dtype == object:
            msg = "masks must be arrays of one shape"
            raise ValueError(msg)
        host = host.astype(bool)
        if host.ndim == 2:
            items = [host]
        elif host.ndim == 3 and frames is not None:
            items = list(host)
        else:
            msg = f"mask must have the frame's shape {shape}, got {host.shape}"
            raise ValueError(msg)
    for m in items:
        if m.ndim != 2 or tuple(m.shape) != shape:
            msg = f"mask must have the frame's shape {shape}, got {tuple(m.shape)}"
            raise ValueError(msg)
    if len(items) != 1 and len(items) != frames:
        msg = f"{len(items)} masks for {frames} frames: pass one mask, or one per frame"
        raise ValueError(msg)
    return on_device, items


def _mask_view(m: "device_array.DeviceArray") -> _native.View:
    """rpsf_view of a 2-D uint8 device mask (an axis of length one may carry any stride: it is never stepped along)."""
    return _native.View(m.ptr or None, _native.DTYPES["|u1"], m.shape[0], m.shape[1], max(1, m.strides[0]), max(1, m.strides[1]))


def _pad_mask(mask: np.ndarray | None, shape, n: int, pad_mode) -> np.ndarray:
    """The caller's mask on the 2N-padded frame: through the pad mode's index map where there is one, False in the pad otherwise."""
    if mask is None:
        return np.zeros((shape[0] + 4 * n, shape[1] + 4 * n), bool)
    if isinstance(pad_mode, str) and pad_mode in _INDEX_MAP_MODES:
        return np.pad(mask, 2 * n, mode=pad_mode)
    return np.pad(mask, 2 * n, mode="constant", constant_values=False)


class ArrayPSFTransform:
    """Transformation from a source PSF to a target PSF that can be applied to images."""

    def __init__(self, transfer_kernel: IndexedCube, device: int = 0, *, saturation: str = "host") -> None:
        self._transfer_kernel = transfer_kernel
        self._device = device
        self.saturation = saturation
        self._plan: _native.Plan | None = None
        self._plan_stamp: tuple | None = None
        self._corner_bounds: tuple | None = None
        self.last_route = 0  # RPSF_ROUTE_* bits of the last apply / apply_batch on device arrays (include/rpsf.h)
        # one device plan (staging buffers, colour planes, one stream) per transform: calls from several threads take turns
        self._lock = threading.RLock()

    # ------------------------------------------------------------------ accessors (transform.py:37-51)
    @property
    def psf_shape(self) -> tuple[int, int]:
        return self._transfer_kernel.sample_shape

    @property
    def coordinates(self) -> list[tuple[int, int]]:
        return self._transfer_kernel.coordinates

    def __len__(self) -> int:
        return len(self._transfer_kernel)

    def __eq__(self, other: object) -> bool:
        if not isinstance(other, ArrayPSFTransform):
            msg = "Can only compare ArrayPSFTransform to another ArrayPSFTransform."
            raise TypeError(msg)
        return self._transfer_kernel == other._transfer_kernel

    __hash__ = None

    @property
    def saturation(self) -> str:
        """Where ``apply`` does the steps of the saturation branch around the correction (mask, dilation, ordered fill, restore):
        ``"host"`` (default) as the reference does them, on the float64 frame, or ``"device"``: kernels F1 - F5 on the float32 frame
        (DESIGN.md 3.8).  Bit-identical on float32 frames; not in the reference's API."""
        return self._saturation

    @saturation.setter
    def saturation(self, value: str) -> None:
        if value not in ("host", "device"):
            msg = f"saturation must be 'host' or 'device', got {value!r}"
            raise ValueError(msg)
        self._saturation = value

    # ------------------------------------------------------------------ construct (transform.py:53-83)
    @classmethod
    def construct(cls, source, target, alpha: float, epsilon: float, device: int = 0, *, saturation: str = "host") -> "ArrayPSFTransform":
        """Build the transform taking ``source`` to ``target``.

        ``alpha`` controls the hardness of the transition from amplification to attenuation and
        ``epsilon`` the maximum amplification.  Raises :class:`InvalidCoordinateError` when the two
        models are not sampled at the same coordinates (transform.py:74-76).  The kernel keeps the
        dtype of the PSF spectra (complex64 for float32 PSFs, complex128 for float64 ones).
        ``saturation`` (keyword only, not in the reference): see the property of that name.
        """
        if np.any(np.array(source.coordinates) != np.array(target.coordinates)):
            msg = "Source PSF coordinates do not match target PSF coordinates."
            raise InvalidCoordinateError(msg)
        n_patch = source.sample_shape[0] if len(source) else 0
        dev_s, dev_t = getattr(source, "_fft_dev", None), getattr(target, "_fft_dev", None)

        def pristine(psf) -> bool:
            # the device copy of the spectra is what the reference would use only while nobody has fetched the cube (a fetched
            # array can be edited in place: transform.py:78-82 reads fft_evaluations as they are at the time of the call)
            cube = getattr(psf, "_fft_cube", None)
            return cube is not None and getattr(cube, "_loader", None) is not None and cube._edits == 0

        if (dev_s is not None and dev_t is not None and pristine(source) and pristine(target)
                and dev_s[1] == dev_t[1] == device and len(source) == len(target) > 0
                and source.sample_shape == target.sample_shape and n_patch in _native.SUPPORTED_PATCH_SIZES
                and all(isinstance(v, numbers.Integral) for c in source.coordinates for v in c)):
            # Both spectra were computed on this GPU (ArrayPSF(device=...)) and are still there: K2 -> pack -> plan without
            # anything crossing PCIe; the IndexedCube downloads K the first time somebody looks at its values.
            # spectra -> packed K in ONE pass (the formula is evaluated where the packer reads K): the full K - 571 MB at 1089 patches of 256
            # pixels - is neither written nor read back; it is built, from the same resident spectra, only if somebody looks at the values.
            count = len(source) * n_patch * n_patch
            plan = _native.Plan(n_patch, source.coordinates, device=device)
            plan.set_transfer_spectra_device(dev_s[0].ptr, dev_t[0].ptr, alpha, epsilon)
            shape = (len(source), n_patch, n_patch)

            def fetch(bufs=(dev_s[0], dev_t[0]), shape=shape, count=count):  # (holds the two spectra alive)
                kbuf = _native.DeviceBuffer(count * 8, device)
                try:
                    _native.build_transfer_device(bufs[0].ptr, bufs[1].ptr, kbuf.ptr, count, False, alpha, epsilon, device)
                    return kbuf.download(shape, np.complex64)
                finally:
                    kbuf.free()

            cube = IndexedCube._deferred(source.coordinates, shape, fetch)
            out = cls(cube, device=device, saturation=saturation)
            out._plan, out._plan_stamp = plan, _kernel_stamp(cube)
            ref = weakref.ref(out)

            def fetched(c, stamp=out._plan_stamp):
                # looking at K must not cost a re-upload: the values that just arrived ARE the device copy
                t = ref()
                if t is not None and t._plan_stamp == stamp:
                    t._plan_stamp = _kernel_stamp(c)

            cube._load_hook = fetched
            return out
        s_fft, t_fft = source.fft_evaluations, target.fft_evaluations
        resident = (np.result_type(s_fft.dtype, t_fft.dtype) == np.complex64 and s_fft.ndim == 3 and len(source) > 0
                    and s_fft.shape == t_fft.shape and s_fft.shape[1] == s_fft.shape[2]
                    and s_fft.shape[1] in _native.SUPPORTED_PATCH_SIZES
                    and all(isinstance(v, numbers.Integral) for c in source.coordinates for v in c))
        if not resident:
            kernel = _native.build_transfer(s_fft, t_fft, alpha, epsilon, device=device)
            return cls(IndexedCube(source.coordinates, kernel), device=device, saturation=saturation)
        # complex64 spectra and a patch size the kernels support: K is built on the device, packed for K1 from
        # there (no second trip over PCIe at the first apply) and copied back once for the IndexedCube.
        s_fft = np.ascontiguousarray(s_fft, dtype=np.complex64)
        t_fft = np.ascontiguousarray(t_fft, dtype=np.complex64)
        bufs = [_native.DeviceBuffer(s_fft.nbytes, device) for _ in range(3)]
        try:
            bufs[0].upload(s_fft)
            bufs[1].upload(t_fft)
            _native.build_transfer_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, s_fft.size, False, alpha, epsilon, device)
            plan = _native.Plan(s_fft.shape[1], source.coordinates, device=device)
            plan.set_transfer_device(bufs[2].ptr)
            plan.synchronize()
            kernel = bufs[2].download(s_fft.shape, np.complex64)
        finally:
            for b in bufs:
                b.free()
        cube = IndexedCube(source.coordinates, kernel)
        out = cls(cube, device=device, saturation=saturation)
        out._plan, out._plan_stamp = plan, _kernel_stamp(cube)
        return out

    # ------------------------------------------------------------------ device plan
    def invalidate(self) -> None:
        """Drop the device copy of the transfer kernel; ``values`` becomes writeable again (it was made read-only when the copy was
        taken).  The next ``apply`` uploads whatever the array holds then - the reference reads ``values`` at every apply (transform.py:164)."""
        with self._lock:
            if self._plan is not None:
                self._plan.close()
            self._plan, self._plan_stamp = None, None
            self._thaw()

    def _freeze(self) -> None:
        """A device copy of ``values`` exists: make the array read-only, so that an in-place edit raises instead of leaving the copy stale."""
        cube = self._transfer_kernel
        values = cube._values_array
        if values is not None and values.flags.writeable:
            try:
                values.flags.writeable = False
                cube._frozen = True
            except ValueError:  # (an array that does not own its memory and whose base forbids it: the fingerprint remains)
                pass

    def _thaw(self) -> None:
        cube = self._transfer_kernel
        if getattr(cube, "_frozen", False) and cube._values_array is not None:
            cube._values_array.flags.writeable = True
            cube._frozen = False

    def edit(self):
        """``with transform.edit() as k: k[i, r, c] = x`` - the transfer kernel's array, writeable inside the block; the device copy is
        refreshed at the next ``apply`` (every edit made this way is seen, however small)."""
        import contextlib

        @contextlib.contextmanager
        def editing():
            with self._lock:
                cube = self._transfer_kernel
                values = cube.values
                self._thaw()
                try:
                    yield values
                finally:
                    cube._edits += 1  # the stamp changes: the next apply uploads the array again (and makes it read-only again)

        return editing()

    def _checked_patch_size(self) -> int:
        n0, n1 = self.psf_shape
        if n0 != n1:
            msg = f"operands could not be broadcast together: PSF samples must be square, got {self.psf_shape}"
            raise ValueError(msg)
        if not 2 <= n0 <= 4096:  # 16..256 (powers of two) run the hand-written kernels, the rest the hipFFT fallback
            msg = f"patch size {n0} is outside the supported range 2..4096"
            raise NotImplementedError(msg)
        return n0

    def _device_plan(self) -> _native.Plan:
        cube = self._transfer_kernel
        stamp = _kernel_stamp(cube)
        if self._plan is None or self._plan_stamp != stamp:
            self.invalidate()
            n = self._checked_patch_size()
            for coordinate in cube.coordinates:  # the reference slices with these (transform.py:141-149)
                if not all(isinstance(v, numbers.Integral) for v in coordinate):
                    msg = "slice indices must be integers: patch coordinates must be integral"
                    raise TypeError(msg)
            plan = _native.Plan(n, cube.coordinates, device=self._device)
            plan.set_transfer(cube.values)
            self._plan, self._plan_stamp = plan, stamp
        self._freeze()
        return self._plan

    def _check_corners(self, n: int, height: int, width: int) -> None:
        """Outside the 2N pad the reference's np.stack is ragged -> ValueError (transform.py:141-162)."""
        coords = self.coordinates
        if self._corner_bounds is None or self._corner_bounds[0] != len(coords):  # extremes, once per corner list
            arr = np.asarray(coords).reshape(-1, 2)
            self._corner_bounds = (len(coords), arr[:, 0].min(), arr[:, 0].max(), arr[:, 1].min(), arr[:, 1].max())
        _, rlo, rhi, clo, chi = self._corner_bounds
        if rlo < -2 * n or rhi > height + n or clo < -2 * n or chi > width + n:
            bad = next((r, c) for r, c in coords if r < -2 * n or r > height + n or c < -2 * n or c > width + n)
            msg = f"patch corner {bad} lies outside the padded image"
            raise ValueError(msg)

    # ------------------------------------------------------------------ apply (transform.py:85-177)
    def apply(self, image: np.ndarray, workers: int | None = None, pad_mode: str = "symmetric",
              saturation_threshold: float = math.inf, saturation_dilation: int = 1,
              neighborhood_width: int = 7, *, out: np.ndarray | None = None, stream=None, mask=None,
              fill_nonfinite: bool = False) -> np.ndarray:
        """Apply the transform to an image and return the corrected image (float64, same shape).

        Parameters follow the reference: ``pad_mode`` is any ``np.pad`` mode; pixels brighter than
        ``saturation_threshold`` are replaced by their neighbourhood mean before correction and
        restored afterwards.  ``workers`` is accepted for compatibility and ignored (the FFTs run
        on the GPU).  The input is never modified.

        ``out`` (keyword only, not in the reference): a C-contiguous float64 or float32 array of the image's shape to write the result
        into and return - a caller's loop that reuses one result array spares every call the first touch of two megabytes of fresh pages
        per 512 x 512 frame, which costs anything between 10 and 200 us on a busy host (`scripts/notebook_factors.py`).

        DEVICE FRAMES (not in the reference): ``image`` may be a :class:`~regularizepsf_amd.DeviceArray`, or any object with
        ``__cuda_array_interface__``, on the transform's device - float32, float64, float16, uint8, int16, uint16 or int32, at any
        positive strides.  The result is then a ``DeviceArray`` and nothing crosses PCIe.  ITS DTYPE IS ``out``'s IF ``out`` IS GIVEN, ELSE
        FLOAT32 - not the float64 of the host route: the kernels compute in float32, and widening a resident frame would only double its
        bytes.  ``out`` may be a float32, float64 or float16 device array (or protocol object) of the image's shape at any positive strides;
        it is returned itself when it is a ``DeviceArray``, wrapped in one otherwise.  A float32 side whose rows are contiguous
        (any row pitch, any offset) is read or written in place; every other side goes through a conversion kernel and staging owned by
        the plan.  Integer and float64 frames enter as ``(float)(double)v``, so the result is that of the host route on
        ``image.astype(np.float32)``.  A finite ``saturation_threshold`` runs the saturation kernels on the device whatever
        ``saturation=`` says.
        ``stream=None`` is the safe mode: the call waits for the device before it launches (whoever produced ``image`` is unknown) and for
        its own stream before it returns.  ``stream=`` an integer stream handle, or an object with a ``cuda_stream`` attribute, is the
        asynchronous mode: everything is enqueued on that stream, behind the stream the input says it was last written on (an event),
        the call does not wait on the host (the saturation route does once, for its counts) and the result carries the stream until
        ``to_host`` has waited for it.
        What the device routes do not cover comes down, runs the host route above and goes back up, cast to the result dtype:
        ``np.pad`` modes the kernels do not evaluate (anything but constant, symmetric, reflect, edge, wrap) and the corner cases of the
        saturation arguments (a threshold that is not finite, ``saturation_dilation < 1`` or not integral, ``neighborhood_width // 2 < 1``).

        BAD PIXELS (keyword only, not in the reference): ``mask`` names pixels to treat as the saturated ones are -
        replaced by the mean of their neighbourhood before the correction, returned as the caller's own values after it - without being
        brighter than anything: an array of the image's shape, nonzero = masked; a NumPy array of any dtype ``astype(bool)`` takes, or,
        with a device frame, a uint8 ``DeviceArray`` / ``__cuda_array_interface__`` object at any positive strides (a NumPy mask with a
        device frame is uploaded; a device mask with a NumPy frame is a ``TypeError``).  ``fill_nonfinite=True`` treats every NaN and
        +-Inf pixel of the frame so.  Unlike the pixels above ``saturation_threshold`` these are NOT dilated: the mask goes onto the
        padded frame through the pad mode's index map (symmetric, reflect, edge, wrap; no pad pixel is masked otherwise) and is or-ed
        with the dilated saturation mask.  Either keyword sends the frame down the device saturation route (kernels F1 - F5) whatever
        ``saturation=`` says, also with ``saturation_threshold=inf``; arguments that route does not cover take the NumPy steps of the
        definition.  With both at their defaults nothing changes.  A wrong mask shape or dtype raises ``ValueError`` before any work.
        """
        del workers
        masked = mask is not None or bool(fill_nonfinite)
        if device_array.is_device_array(image):
            with self._lock:
                if masked:
                    return self._apply_device_locked(image, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, out, stream,
                                                     mask, True, bool(fill_nonfinite))
                return self._apply_device_locked(image, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, out, stream)
        if stream is not None:
            msg = "stream= goes with device arrays; a NumPy frame is corrected when the call returns"
            raise ValueError(msg)
        with self._lock:
            if masked:
                result = self._apply_locked(image, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, out, mask, True,
                                            bool(fill_nonfinite))
            else:
                result = self._apply_locked(image, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, out)
        if out is not None and result is not out:  # (the branches that build their result on the host)
            if out.shape != result.shape:
                msg = "out must have the image's shape"
                raise ValueError(msg)
            out[...] = result
            return out
        return result

    def _apply_locked(self, image, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, out=None, mask=None, masked=False,
                      fill_nonfinite=False) -> np.ndarray:
        """``masked``: the call names bad pixels (``mask``: what the caller gave, or a checked bool array; ``fill_nonfinite``)."""
        image = np.asarray(image)
        if image.ndim != 2:
            msg = f"image must be two dimensional, got shape {image.shape}"
            raise ValueError(msg)
        if masked:
            _, items = _check_masks(mask, image.shape, None, self._device, False)
            mask = items[0] if items else None
        if len(self) == 0:  # the reference fails in np.stack([]) (transform.py:157-162)
            msg = "need at least one array to stack"
            raise ValueError(msg)
        n = self._checked_patch_size()
        plan = self._device_plan()
        height, width = image.shape
        self._check_corners(n, height, width)

        if masked and self._device_route(pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, masked=True):
            # F1 - F5 with the exact plane (rpsf_apply_frames_host_masked_device, a frame-group of one); a float64 frame gets its own bits back on the mask
            return plan.apply_frames_host_masked_device([image], _native.PAD_MODES[pad_mode], saturation_threshold, saturation_dilation,
                                                        neighborhood_width, None if mask is None else [mask], fill_nonfinite)[0]

        if not masked and saturation_threshold == math.inf and pad_mode in _native.PAD_MODES:  # nothing can exceed +inf
            return plan.apply_host(image, _native.PAD_MODES[pad_mode], out=out)  # float64 out (or the caller's array); conversions inside the library

        if (not masked and pad_mode in _native.PAD_MODES and isinstance(saturation_dilation, numbers.Integral) and saturation_dilation >= 1
                and isinstance(neighborhood_width, numbers.Integral) and neighborhood_width >= 0):
            # the saturation branch in one library call: the reference's host steps (pad, mask, dilation, sequential fill, restore) on the
            # plan's own scratch, the correction of the padded frame on the GPU (rpsf_apply_host_saturated)
            if self._saturation == "device" and neighborhood_width // 2 >= 1:
                # the same steps on the GPU, on the float32 frame (rpsf_apply_host_saturated_device); an always-empty window stays with the host
                return plan.apply_host_saturated_device(image, _native.PAD_MODES[pad_mode], saturation_threshold, saturation_dilation,
                                                        neighborhood_width)
            return plan.apply_host_saturated(image, _native.PAD_MODES[pad_mode], saturation_threshold, saturation_dilation,
                                             neighborhood_width)

        # Host-side padding: np.pad modes the kernel does not evaluate, and the corner cases of the saturation branch (dilation < 1: scipy
        # iterates to a fixed point; negative widths), which work on the padded image (transform.py:119-138,171-172).
        padded = np.pad(image.astype(float), ((2 * n, 2 * n), (2 * n, 2 * n)), mode=pad_mode)
        raw = padded.copy()
        bad = mask
        mask = padded > saturation_threshold
        if np.any(mask):
            from scipy.ndimage import binary_dilation

            mask = binary_dilation(mask, iterations=saturation_dilation)
        if masked:  # the pixels masked as they are: not dilated ("Bad-pixel masks")
            exact = _pad_mask(bad, image.shape, n, pad_mode)
            if fill_nonfinite:
                exact |= ~np.isfinite(padded)
            mask = mask | exact
        if np.any(mask):
            padded[mask] = np.nan
            if neighborhood_width >= 0:
                # the reference's per-pixel np.nanmean loop, restated in C (same order, same window rule)
                _native.saturation_fill(padded, mask, neighborhood_width)
            else:  # negative widths: keep NumPy's own slice arithmetic
                half = neighborhood_width // 2
                with np.errstate(all="ignore"):
                    for i, j in zip(*np.where(mask)):
                        padded[i, j] = np.nanmean(padded[i - half : i + half, j - half : j + half])
        corrected = self._apply_prepadded(padded.astype(np.float32), 2 * n)
        corrected = corrected.astype(np.float64)
        corrected[mask] = raw[mask]
        return corrected[2 * n : height + 2 * n, 2 * n : width + 2 * n]

    # ------------------------------------------------------------------ device frames
    def _device_route(self, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, masked=False) -> bool:
        """Whether rpsf_apply_view / rpsf_apply_batch_view cover these arguments (else: down, the host route, up).  ``masked``: the
        saturation kernels run whatever the threshold, so their preconditions hold for +inf as well."""
        if pad_mode not in _native.PAD_MODES or not isinstance(saturation_threshold, numbers.Real):
            return False
        if saturation_threshold == math.inf and not masked:
            return True
        return ((math.isfinite(saturation_threshold) or saturation_threshold == math.inf) and isinstance(saturation_dilation, numbers.Integral) and saturation_dilation >= 1
                and isinstance(neighborhood_width, numbers.Integral) and neighborhood_width // 2 >= 1)

    def _enter_stream(self, stream, inputs, outputs):
        """Order a device call behind what is pending on its arrays; returns (handle or None, c_void_p or None)."""
        handle = device_array.stream_handle(stream)
        if handle is None:  # the safe mode: nobody knows what produced the input, or on which stream
            _native.check(_native.lib().rpsf_device_synchronize(self._device))
            for a in (*inputs, *outputs):
                a._pending.stream = None
            return None, None
        s = _native.c_void_p(handle)
        for pending in {a._pending.stream for a in (*inputs, *outputs)} - {None, handle}:
            _native.stream_wait(s, _native.c_void_p(pending), self._device)
        return handle, s

    def _leave_stream(self, plan, handle, outputs) -> None:
        if handle is None:
            _native.stream_synchronize(plan.stream, self._device)
        for a in outputs:
            a._pending.stream = handle

    def _device_out(self, out, shape, dtype) -> "device_array.DeviceArray":
        if out is None:
            return device_array.device_empty(shape, dtype, self._device)
        out = device_array.as_device_array(out, self._device, writeable=True, what="out")
        if out.dtype not in device_array.RESULT_DTYPES:
            msg = f"out must be float32, float64 or float16, got {out.dtype}"
            raise ValueError(msg)
        if out.shape != tuple(shape):
            msg = "out must have the image's shape"
            raise ValueError(msg)
        return out

    def _apply_device_locked(self, image, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, out, stream, mask=None,
                             masked=False, fill_nonfinite=False):
        image = device_array.as_device_array(image, self._device)
        if image.ndim != 2:
            msg = f"image must be two dimensional, got shape {image.shape}"
            raise ValueError(msg)
        mask_on_device = False
        if masked:
            mask_on_device, items = _check_masks(mask, image.shape, None, self._device, True)
            mask = items[0] if items else None
        if len(self) == 0:
            msg = "need at least one array to stack"
            raise ValueError(msg)
        n = self._checked_patch_size()
        plan = self._device_plan()
        self._check_corners(n, *image.shape)
        result = self._device_out(out, image.shape, np.float32)
        if not self._device_route(pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, masked):
            if masked:
                host = self._apply_locked(image.to_host(), pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, None,
                                          mask.to_host() if mask_on_device else mask, True, fill_nonfinite)
            else:
                host = self._apply_locked(image.to_host(), pad_mode, saturation_threshold, saturation_dilation, neighborhood_width)
            result._assign(host.astype(result.dtype))
            return result
        if masked and mask is not None and not mask_on_device:
            mask = device_array.to_device(mask.astype(np.uint8), self._device)  # (F1 has read it when the call returns: the route's one wait comes later)
        handle, s = self._enter_stream(stream, (image,) if mask is None else (image, mask), (result,))
        if masked:
            self.last_route = plan.apply_view_masked(image._view2d(), result._view2d(), _native.PAD_MODES[pad_mode], saturation_threshold,
                                                     saturation_dilation, neighborhood_width, None if mask is None else _mask_view(mask),
                                                     fill_nonfinite, s)
        else:
            self.last_route = plan.apply_view(image._view2d(), result._view2d(), _native.PAD_MODES[pad_mode], saturation_threshold,
                                              saturation_dilation, neighborhood_width, s)
        self._leave_stream(plan, handle, (result,))
        return result

    def _apply_batch_device_locked(self, images, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, dtype, out, stream,
                                   mask=None, masked=False, fill_nonfinite=False):
        if device_array.is_device_array(images):
            stack = device_array.as_device_array(images, self._device, what="images")
            if stack.ndim != 3:
                msg = f"images must have shape (frames, H, W), got {stack.shape}"
                raise ValueError(msg)
            frames, shape = [stack[i] for i in range(stack.shape[0])], stack.shape[1:]
        else:
            frames = [device_array.as_device_array(im, self._device, what="images") for im in images]
            shape = frames[0].shape if frames else (0, 0)
            if any(f.ndim != 2 or f.shape != shape for f in frames):
                msg = "images must be a sequence of two dimensional arrays of one shape"
                raise ValueError(msg)
        dtype = np.dtype(dtype)
        if out is not None:
            out = device_array.as_device_array(out, self._device, writeable=True, what="out")
            dtype = out.dtype
            if out.shape != (len(frames), *shape):
                msg = "out must have shape (frames, H, W)"
                raise ValueError(msg)
        masks, masks_on_device = None, False
        if masked:
            masks_on_device, masks = _check_masks(mask, shape, len(frames), self._device, True)
        covered = (dtype in device_array.RESULT_DTYPES and len(frames) > 0
                   and self._device_route(pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, masked))
        if not covered:  # down, the host route, up: the host route's result, whatever it is for these arguments
            bad = ()
            if masked:
                bad = (None if masks is None else [m.to_host() if masks_on_device else m for m in masks], True, fill_nonfinite)
            host = self._apply_batch_locked([f.to_host() for f in frames], None, pad_mode, saturation_threshold, saturation_dilation,
                                            neighborhood_width, dtype if dtype in device_array.RESULT_DTYPES else np.float64, None, *bad)
            if out is None:
                return device_array.to_device(host.astype(dtype if dtype in device_array.DTYPES else np.float64, copy=False), self._device)
            out._assign(host)
            return out
        if len(self) == 0:
            msg = "need at least one array to stack"
            raise ValueError(msg)
        n = self._checked_patch_size()
        plan = self._device_plan()
        self._check_corners(n, *shape)
        result = out if out is not None else device_array.device_empty((len(frames), *shape), dtype, self._device)
        if masks is not None and not masks_on_device:  # one upload for the call (F1 has read it when the call returns)
            stack = device_array.to_device(np.stack(masks).astype(np.uint8), self._device)
            masks = [stack[i] for i in range(len(masks))]
        handle, s = self._enter_stream(stream, (*frames, *(masks or ())), (result,))
        if masked:
            self.last_route = plan.apply_batch_view_masked([f._view2d() for f in frames], [result[i]._view2d() for i in range(len(frames))],
                                                           _native.PAD_MODES[pad_mode], saturation_threshold, saturation_dilation,
                                                           neighborhood_width, None if masks is None else [_mask_view(m) for m in masks],
                                                           fill_nonfinite, s)
        else:
            self.last_route = plan.apply_batch_view([f._view2d() for f in frames], [result[i]._view2d() for i in range(len(frames))],
                                                    _native.PAD_MODES[pad_mode], saturation_threshold, saturation_dilation, neighborhood_width, s)
        self._leave_stream(plan, handle, (result,))
        return result

    def _apply_prepadded(self, padded: np.ndarray, shift: int) -> np.ndarray:
        """Run K1 on an image the host already padded by ``shift`` on every side (constant mode, shifted corners)."""
        plan = self._device_plan()
        h, w = padded.shape
        img = _native.DeviceBuffer(padded.nbytes, self._device).upload(padded)
        out = _native.DeviceBuffer(padded.nbytes, self._device)
        try:
            geom = _native.Geometry.whole(h, w, _native.PAD_MODES["constant"], 0.0)
            geom.origin_row = geom.origin_col = shift
            plan.apply_device(img.ptr, out.ptr, geom)
            plan.synchronize()
            return out.download((h, w))
        finally:
            img.free()
            out.free()

    #: pre-1.0 name of :meth:`apply` (the task description refers to it)
    correct_image = apply

    def apply_batch(self, images, workers: int | None = None, pad_mode: str = "symmetric",
                    saturation_threshold: float = math.inf, saturation_dilation: int = 1,
                    neighborhood_width: int = 7, dtype: type = np.float64, out: np.ndarray | None = None, stream=None, *, mask=None,
                    fill_nonfinite: bool = False) -> np.ndarray:
        """Apply the transform to a stack ``(frames, H, W)`` or a sequence of equally shaped images; returns a stack.

        Equivalent to ``np.stack([self.apply(im, ...) for im in images])`` - the loop a user of the reference writes
        (docs/source/example.ipynb over transform.py:85-177) - and bit-identical to it, but streamed: while one group
        of frames is corrected, the next one crosses PCIe to the device and the previous one comes back and is widened to
        float64, on three streams and a persistent pool of host threads (``rpsf_apply_frames_host``).  Frames that already
        live on the GPU are passed as they are: a 3-D :class:`~regularizepsf_amd.DeviceArray` (or object with
        ``__cuda_array_interface__``) or a sequence of 2-D ones, with ``out=`` a 3-D one and ``stream=`` as in :meth:`apply`; the result is
        a ``DeviceArray`` of ``dtype`` (float32, float64 or float16 on the device routes) and each frame has the bits of :meth:`apply` on it.
        Mixing host and device frames in one sequence raises ``ValueError``.  ``dtype`` is the result dtype (the reference
        returns float64; ``np.float32`` skips the widening); ``out`` an existing C-contiguous stack to fill.
        With a finite ``saturation_threshold`` and ``saturation="device"``, float32 / float64 frames go through the batched device route
        (``rpsf_apply_frames_host_saturated_device``: the frames of a frame-group share the launches of kernels F1 - F3, the host waits for
        the device once and one launch fills every frame's groups), again bit-identical to the loop.
        ``mask`` and ``fill_nonfinite`` (keyword only) are :meth:`apply`'s: ``mask`` is one 2-D mask for all frames, or one per frame as a
        3-D stack or a sequence (NumPy, or uint8 device arrays with device frames).  The frames of a frame-group share the masked
        launches as they share the saturation ones (``rpsf_apply_frames_host_masked_device``, ``rpsf_apply_batch_view_masked``).
        Extension of the reference API - there is no ``apply_batch`` upstream.
        """
        masked = mask is not None or bool(fill_nonfinite)
        bad = (mask, True, bool(fill_nonfinite)) if masked else ()
        on_device = device_array.is_device_array(images)
        if not on_device and not isinstance(images, np.ndarray):
            images = list(images)
            kinds = {device_array.is_device_array(im) for im in images}
            if len(kinds) == 2:
                msg = "images mixes host and device frames"
                raise ValueError(msg)
            on_device = kinds == {True}
        if on_device:
            with self._lock:
                return self._apply_batch_device_locked(images, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width,
                                                       dtype, out, stream, *bad)
        if stream is not None:
            msg = "stream= goes with device arrays; NumPy frames are corrected when the call returns"
            raise ValueError(msg)
        with self._lock:
            return self._apply_batch_locked(images, workers, pad_mode, saturation_threshold, saturation_dilation,
                                            neighborhood_width, dtype, out, *bad)

    def _apply_batch_locked(self, images, workers, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width,
                            dtype, out, mask=None, masked=False, fill_nonfinite=False) -> np.ndarray:
        stack = None
        if isinstance(images, np.ndarray):
            if images.ndim != 3:
                msg = f"images must have shape (frames, H, W), got {images.shape}"
                raise ValueError(msg)
            frames = images  # (iterated only on the per-frame routes below)
            stack = images
            shape = images.shape[1:]
        else:
            frames = [np.asarray(im) for im in images]
            shape = frames[0].shape if frames else (0, 0)
            if any(f.ndim != 2 or f.shape != shape for f in frames):
                msg = "images must be a sequence of two dimensional arrays of one shape"
                raise ValueError(msg)
        dtype = np.dtype(out.dtype if out is not None else dtype)
        if masked:
            _, masks = _check_masks(mask, shape, len(frames), self._device, False)
            if (self._device_route(pad_mode, saturation_threshold, saturation_dilation, neighborhood_width, masked=True) and len(frames) > 0
                    and len(self) > 0 and dtype in (np.float32, np.float64)):
                # every frame of a frame-group through the masked launches (rpsf_apply_frames_host_masked_device); the bits of the loop over apply
                n = self._checked_patch_size()
                plan = self._device_plan()
                self._check_corners(n, *shape)
                res = plan.apply_frames_host_masked_device(frames, _native.PAD_MODES[pad_mode], saturation_threshold, saturation_dilation,
                                                           neighborhood_width, masks, fill_nonfinite, out_dtype=dtype)
            else:
                outs = [self.apply(im, workers, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width,
                                   mask=None if masks is None else masks[i if len(masks) > 1 else 0], fill_nonfinite=fill_nonfinite)
                        for i, im in enumerate(frames)]
                res = np.stack(outs).astype(dtype, copy=False) if outs else np.empty((0, *shape), dtype)
            if out is not None:
                out[...] = res
                return out
            return res
        if (self._saturation == "device" and isinstance(saturation_threshold, numbers.Real) and math.isfinite(saturation_threshold)
                and pad_mode in _native.PAD_MODES and len(frames) > 0 and len(self) > 0 and dtype in (np.float32, np.float64)
                and isinstance(saturation_dilation, numbers.Integral) and saturation_dilation >= 1
                and isinstance(neighborhood_width, numbers.Integral) and neighborhood_width // 2 >= 1
                and all(f.dtype in (np.float32, np.float64) for f in ([stack] if stack is not None else frames))):
            # the device route for all frames of a frame-group at once: shared launches of F1 - F3, one host wait, one F4 launch, the shared-K
            # batch launch on the padded frames (rpsf_apply_frames_host_saturated_device); bit-identical to the loop over apply
            n = self._checked_patch_size()
            plan = self._device_plan()
            self._check_corners(n, *shape)
            res = plan.apply_frames_host_saturated_device(frames, _native.PAD_MODES[pad_mode], saturation_threshold, saturation_dilation,
                                                          neighborhood_width, out_dtype=dtype)
            if out is not None:
                out[...] = res
                return out
            return res
        if (saturation_threshold != math.inf and pad_mode in _native.PAD_MODES and len(frames) > 0 and len(self) > 0
                and dtype in (np.float32, np.float64) and isinstance(saturation_dilation, numbers.Integral) and saturation_dilation >= 1
                and isinstance(neighborhood_width, numbers.Integral) and neighborhood_width >= 0
                and not (self._saturation == "device" and neighborhood_width // 2 >= 1)):  # (the device route's other frames - integer frames, a threshold that is not finite: the loop over apply, below)
            # the saturation branch for a sequence of frames: the host steps of frame i + 1 (pad, mask, dilation, sequential fill) run while the
            # GPU corrects frame i (rpsf_apply_frames_host_saturated)
            n = self._checked_patch_size()
            plan = self._device_plan()
            self._check_corners(n, *shape)
            res = plan.apply_frames_host_saturated(frames, _native.PAD_MODES[pad_mode], saturation_threshold, saturation_dilation,
                                                   neighborhood_width, out_dtype=dtype)
            if out is not None:
                out[...] = res
                return out
            return res
        if (saturation_threshold != math.inf or pad_mode not in _native.PAD_MODES or len(frames) == 0
                or dtype not in (np.float32, np.float64)):
            outs = [self.apply(im, workers, pad_mode, saturation_threshold, saturation_dilation, neighborhood_width)
                    for im in frames]
            res = np.stack(outs).astype(dtype, copy=False) if outs else np.empty((0, *shape), dtype)
            if out is not None:
                out[...] = res
                return out
            return res
        if len(self) == 0:
            msg = "need at least one array to stack"
            raise ValueError(msg)
        n = self._checked_patch_size()
        plan = self._device_plan()
        height, width = shape
        self._check_corners(n, height, width)
        return plan.apply_frames_host(stack if stack is not None else frames, _native.PAD_MODES[pad_mode], out_dtype=dtype, out=out)

    # ------------------------------------------------------------------ persistence (transform.py:220-282)
    def save(self, path: pathlib.Path, overwrite: bool = False) -> None:
        """Save to ``.h5``: datasets ``coordinates`` (n, 2) int64 and ``transfer_kernel`` (n, N, N) complex, exactly
        what the reference writes (``transform.py:236-240``), so either package loads the other's files.
        ``overwrite=False`` raises ``FileExistsError`` for an existing file (h5py mode ``"w-"`` upstream)."""
        path = pathlib.Path(path)
        if path.suffix == ".h5":
            from regularizepsf_amd import _h5min

            _h5min.write_datasets(path, {"coordinates": np.array(self.coordinates, dtype=np.int64).reshape(-1, 2),
                                         "transfer_kernel": self._transfer_kernel.values}, overwrite=overwrite)
        elif path.suffix == ".fits":
            msg = "FITS persistence is not implemented in this package (lossy CompImageHDU semantics live in astropy; see DESIGN.md)"
            raise NotImplementedError(msg)
        else:
            msg = f"Unsupported file type {path.suffix}. Change to .h5 or .fits."
            raise NotImplementedError(msg)

    @classmethod
    def load(cls, path: pathlib.Path, device: int = 0) -> "ArrayPSFTransform":
        """Load a transform saved by this package or by the reference (``transform.py:266-270``)."""
        path = pathlib.Path(path)
        if path.suffix == ".h5":
            from regularizepsf_amd import _h5min

            data = _h5min.read_datasets(path, ["coordinates", "transfer_kernel"])
            coordinates = [tuple(int(v) for v in c) for c in data["coordinates"]]
            return cls(IndexedCube(coordinates, data["transfer_kernel"]), device=device)
        if path.suffix == ".fits":
            msg = "FITS persistence is not implemented in this package (lossy CompImageHDU semantics live in astropy; see DESIGN.md)"
            raise NotImplementedError(msg)
        msg = f"Unsupported file type {path.suffix}. Change to .h5 or .fits."
        raise NotImplementedError(msg)
