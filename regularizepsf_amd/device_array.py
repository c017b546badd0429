"""Arrays that live on the GPU: what ``ArrayPSFTransform.apply`` / ``apply_batch`` take and return when a frame must not cross PCIe.

``DeviceArray`` is a 1-, 2- or 3-D array in ordinary ``hipMalloc`` memory of one device (``_native.DeviceBuffer`` owns it).  It is a
container, not an array library: it can be made (``to_device``, ``device_empty``), sliced into views, handed to the transform and brought
back (``to_host``, ``np.asarray``).  It speaks ``__cuda_array_interface__`` (version 3) in both directions, so the entry points that take
a ``DeviceArray`` take any object with that attribute.  Extension of the reference API - upstream knows NumPy arrays only.  Neither torch
nor cupy is imported here.
"""

from __future__ import annotations

import ctypes
import numbers

import numpy as np

from regularizepsf_amd import _native

__all__ = ["DeviceArray", "to_device", "device_empty"]

#: dtypes a DeviceArray can hold (kernel C1 of csrc/convert.hip reads all of them; results are float32, float64 or float16)
DTYPES = tuple(np.dtype(t) for t in (np.float32, np.float64, np.float16, np.uint8, np.int16, np.uint16, np.int32))
RESULT_DTYPES = tuple(np.dtype(t) for t in (np.float32, np.float64, np.float16))


class _Pending:
    """Shared by every view of one buffer: the stream the last write was enqueued on while that write is pending, else None."""

    __slots__ = ("stream",)

    def __init__(self, stream: int | None = None) -> None:
        self.stream = stream


def stream_handle(stream) -> int | None:
    """``stream=`` of apply: None, an integer handle, a ``c_void_p`` or an object with ``cuda_stream`` (or ``_native.Stream``'s ``ptr``)."""
    if stream is None:
        return None
    if isinstance(stream, numbers.Integral):
        return int(stream) or None
    if isinstance(stream, ctypes.c_void_p):
        return stream.value or None
    for name in ("cuda_stream", "ptr"):
        if hasattr(stream, name):
            return stream_handle(getattr(stream, name))
    msg = f"stream must be an integer handle or an object with a cuda_stream attribute, got {type(stream).__name__}"
    raise TypeError(msg)


def _c_strides(shape, itemsize: int) -> tuple:
    strides, step = [], itemsize
    for n in reversed(shape):
        strides.append(step)
        step *= max(1, n)
    return tuple(reversed(strides))


class DeviceArray:
    """A 1-, 2- or 3-D array in device memory.  Make one with :func:`to_device` or :func:`device_empty`; index it with integers and
    slices of positive step to get views that share (and keep alive) the buffer: pitched, offset, column-strided, row windows."""

    __slots__ = ("ptr", "shape", "dtype", "strides", "device", "_owner", "_pending")

    def __init__(self, *_args, **_kwargs) -> None:
        msg = "use to_device() or device_empty()"
        raise TypeError(msg)

    @classmethod
    def _from_parts(cls, ptr: int, shape, dtype, strides=None, owner=None, device: int = 0, pending: _Pending | None = None) -> "DeviceArray":
        """(ptr, shape, dtype, strides in bytes or None for C order, whatever keeps the memory alive)."""
        self = object.__new__(cls)
        self.ptr = int(ptr)
        self.shape = tuple(int(n) for n in shape)
        self.dtype = np.dtype(dtype)
        self.strides = _c_strides(self.shape, self.dtype.itemsize) if strides is None else tuple(int(s) for s in strides)
        self.device = int(device)
        self._owner = owner
        self._pending = pending if pending is not None else _Pending()
        if self.dtype not in DTYPES or self.dtype.byteorder == ">":
            msg = f"dtype {self.dtype} is not supported on the device (supported: {', '.join(str(d) for d in DTYPES)})"
            raise ValueError(msg)
        if not 1 <= len(self.shape) <= 3 or len(self.strides) != len(self.shape) or any(n < 0 for n in self.shape):
            msg = f"a device array has one, two or three dimensions, got shape {self.shape}"
            raise ValueError(msg)
        if any(s < 0 for s in self.strides):
            msg = "negative strides are not supported"
            raise ValueError(msg)
        if any(s % self.dtype.itemsize for s in self.strides):
            msg = "strides must be multiples of the item size"
            raise ValueError(msg)
        return self

    # ------------------------------------------------------------------ description
    @property
    def ndim(self) -> int:
        return len(self.shape)

    @property
    def size(self) -> int:
        return int(np.prod(self.shape, dtype=np.int64))

    @property
    def nbytes(self) -> int:
        return self.size * self.dtype.itemsize

    @property
    def c_contiguous(self) -> bool:
        return self.size == 0 or all(s == c for n, s, c in zip(self.shape, self.strides, _c_strides(self.shape, self.dtype.itemsize)) if n > 1)

    def __len__(self) -> int:
        return self.shape[0]

    def __repr__(self) -> str:
        return f"DeviceArray(shape={self.shape}, dtype={self.dtype}, strides={self.strides}, device={self.device})"

    @property
    def __cuda_array_interface__(self) -> dict:
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 3,
                "strides": None if self.c_contiguous else self.strides, "stream": self._pending.stream}

    # ------------------------------------------------------------------ views
    def __getitem__(self, index) -> "DeviceArray":
        if not isinstance(index, tuple):
            index = (index,)
        if len(index) > self.ndim:
            msg = f"too many indices for a {self.ndim}-dimensional device array"
            raise IndexError(msg)
        ptr, shape, strides = self.ptr, [], []
        for axis, (n, stride) in enumerate(zip(self.shape, self.strides)):
            item = index[axis] if axis < len(index) else slice(None)
            if isinstance(item, slice):
                if item.step is not None and item.step <= 0:
                    msg = "slices of a device array need a positive step"
                    raise ValueError(msg)
                start, stop, step = item.indices(n)
                ptr += start * stride
                shape.append(len(range(start, stop, step)))
                strides.append(stride * step)
            elif isinstance(item, numbers.Integral):
                i = int(item) + (n if item < 0 else 0)
                if not 0 <= i < n:
                    msg = f"index {int(item)} is out of bounds for axis {axis} with size {n}"
                    raise IndexError(msg)
                ptr += i * stride
            else:
                msg = "a device array is indexed with integers and slices only"
                raise TypeError(msg)
        if not shape:
            msg = "a device array has no scalars: slice, then to_host()"
            raise IndexError(msg)
        return DeviceArray._from_parts(ptr, shape, self.dtype, strides, self._owner, self.device, self._pending)

    # ------------------------------------------------------------------ host <-> device
    def synchronize(self) -> None:
        """Wait for the write that is pending on this array's buffer, if any."""
        if self._pending.stream is not None:
            _native.stream_synchronize(ctypes.c_void_p(self._pending.stream), self.device)
            self._pending.stream = None

    def _span(self) -> int:
        """Bytes from ``ptr`` to the end of the last element."""
        return 0 if self.size == 0 else sum((n - 1) * s for n, s in zip(self.shape, self.strides)) + self.dtype.itemsize

    def _download_span(self) -> np.ndarray:
        raw = np.empty(self._span(), np.uint8)
        if raw.size:
            _native.check(_native.lib().rpsf_memcpy_d2h(self.device, ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(self.ptr), raw.size))
        return raw

    def to_host(self, out: np.ndarray | None = None) -> np.ndarray:
        """The array's logical contents as a NumPy array (into ``out`` if given), after whatever is pending on it has finished."""
        self.synchronize()
        if out is not None and (out.shape != self.shape or out.dtype != self.dtype):
            msg = "out must have the device array's shape and dtype"
            raise ValueError(msg)
        if self.c_contiguous and (out is None or (out.flags.c_contiguous and out.flags.writeable)):
            out = np.empty(self.shape, self.dtype) if out is None else out
            if out.size:
                _native.check(_native.lib().rpsf_memcpy_d2h(self.device, ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(self.ptr), out.nbytes))
            return out
        # a strided view: the bytes it spans come down, its elements are picked on the host
        picked = np.ndarray(self.shape, self.dtype, buffer=self._download_span(), strides=self.strides) if self.size else np.empty(self.shape, self.dtype)
        if out is None:
            return np.ascontiguousarray(picked)
        out[...] = picked
        return out

    def __array__(self, dtype=None, copy=None) -> np.ndarray:
        host = self.to_host()
        return host if dtype is None else host.astype(dtype, copy=False)

    def _assign(self, array: np.ndarray) -> None:
        """Host values into the array's elements and nowhere else (the upload of ``to_device`` and of the host fallbacks of apply)."""
        self.synchronize()
        array = np.ascontiguousarray(np.broadcast_to(np.asarray(array, dtype=self.dtype), self.shape))
        if self.size == 0:
            return
        if self.c_contiguous:
            raw = array
        else:  # a strided view: the bytes it spans come down, take the elements and go back up as they were elsewhere
            raw = self._download_span()
            np.ndarray(self.shape, self.dtype, buffer=raw, strides=self.strides)[...] = array
        _native.check(_native.lib().rpsf_memcpy_h2d(self.device, ctypes.c_void_p(self.ptr), ctypes.c_void_p(raw.ctypes.data), raw.nbytes))

    def _view2d(self) -> _native.View:
        """rpsf_view of a 2-D array."""
        return _native.View(self.ptr or None, _native.DTYPES[self.dtype.str], self.shape[0], self.shape[1], self.strides[0], self.strides[1])


def device_empty(shape, dtype=np.float32, device: int = 0) -> DeviceArray:
    """An uninitialised C-contiguous device array."""
    shape = (int(shape),) if isinstance(shape, numbers.Integral) else tuple(int(n) for n in shape)
    dtype = np.dtype(dtype)
    probe = DeviceArray._from_parts(0, shape, dtype, None, None, device)  # (refuses what cannot be made before anything is allocated)
    buffer = _native.DeviceBuffer(max(1, probe.nbytes), device)
    return DeviceArray._from_parts(buffer.ptr.value, shape, dtype, None, buffer, device)


def to_device(array, device: int = 0) -> DeviceArray:
    """Upload a NumPy array (its dtype is kept)."""
    array = np.asarray(array)
    out = device_empty(array.shape, array.dtype.newbyteorder("=") if array.dtype.byteorder == ">" else array.dtype, device)
    out._assign(array)
    return out


def _device_of(obj) -> int | None:
    """The device a foreign protocol object says it lives on (the protocol's dict has no such entry): torch's ``device.index``, cupy's
    ``device.id``, a plain integer; None when it does not say."""
    dev = getattr(obj, "device", None)
    for value in (dev, getattr(dev, "index", None), getattr(dev, "id", None)):
        if isinstance(value, numbers.Integral) and not isinstance(value, bool):
            return int(value)
    return None


def as_device_array(obj, device: int, *, writeable: bool = False, what: str = "image") -> DeviceArray:
    """``obj`` (a DeviceArray or anything with ``__cuda_array_interface__``) as a DeviceArray on ``device``, without copying: the ``data``,
    ``shape``, ``typestr``, ``strides`` and ``stream`` entries are honoured.  ValueError for negative strides, strides that are no multiple of
    the item size, another device than ``device`` and - for ``writeable`` - a read-only object."""
    if isinstance(obj, DeviceArray):
        found, result = obj.device, obj
    else:
        cai = obj.__cuda_array_interface__
        if cai.get("mask") is not None:
            msg = f"{what}: masked arrays are not supported"
            raise ValueError(msg)
        ptr, readonly = cai["data"]
        if readonly and writeable:
            msg = f"{what} is read-only"
            raise ValueError(msg)
        found = _device_of(obj)
        stream = cai.get("stream")
        result = DeviceArray._from_parts(ptr or 0, cai["shape"], np.dtype(cai["typestr"]), cai.get("strides"), obj,
                                         device if found is None else found, _Pending(int(stream) if stream else None))
    if found is not None and found != device:
        msg = f"{what} lives on device {found}, the transform on device {device}"
        raise ValueError(msg)
    return result


def is_device_array(obj) -> bool:
    return not isinstance(obj, np.ndarray) and hasattr(obj, "__cuda_array_interface__")
