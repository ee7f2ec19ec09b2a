"""Non-blocking HIP streams for tests/test_gpu_stream_order.py: stream-ordered copies and fills on raw device memory, a query, and a
gate -- work that keeps a stream busy for a known while and then ends by itself.

Bound with ctypes to fuif_amd.hip_runtime(), the one HIP runtime the process holds (no second copy is loaded).  Every function gets a
prototype of its own, so that the shared handle's attributes stay what other callers made of them.  Nothing here touches the GPU at
import: a machine without one collects the tests that use it and deselects them."""
import ctypes as C
import math
import time

import numpy as np

import fuif_amd

HIP_SUCCESS = 0
HIP_NOT_READY = 600           # hipErrorNotReady: what hipStreamQuery answers while work is pending
_STREAM_NON_BLOCKING = 1      # hipStreamNonBlocking: no implicit ordering against the null stream
_D2D = 3                      # hipMemcpyDeviceToDevice

_vp = C.c_void_p
_PROTOTYPES = {
    "hipStreamCreateWithFlags": (C.POINTER(_vp), C.c_uint),
    "hipStreamDestroy": (_vp,),
    "hipStreamSynchronize": (_vp,),
    "hipStreamQuery": (_vp,),
    "hipMemcpyAsync": (_vp, _vp, C.c_size_t, C.c_int, _vp),
    "hipMemsetAsync": (_vp, C.c_int, C.c_size_t, _vp),
    "hipGetLastError": (),
    "hipDeviceSynchronize": (),
    "hipEventCreate": (C.POINTER(_vp),),
    "hipEventRecord": (_vp, _vp),
    "hipEventSynchronize": (_vp,),
    "hipEventElapsedTime": (C.POINTER(C.c_float), _vp, _vp),
    "hipEventDestroy": (_vp,),
}


class Hip:
    """the handful of runtime calls the stream tests need; a stream or an event is a plain integer handle (None = the null stream)"""

    def __init__(self):
        rt = fuif_amd.hip_runtime()
        self.L = fuif_amd.lib()
        self.f = {name: C.CFUNCTYPE(C.c_int, *args)((name, rt)) for name, args in _PROTOTYPES.items()}

    def _ok(self, name, *args):
        rc = self.f[name](*args)
        assert rc == HIP_SUCCESS, "%s: HIP error %d" % (name, rc)

    # ---- streams ----
    def stream(self):
        s = _vp()
        self._ok("hipStreamCreateWithFlags", C.byref(s), _STREAM_NON_BLOCKING)
        assert s.value
        return s.value

    def destroy(self, stream):
        self._ok("hipStreamDestroy", stream)

    def sync(self, stream):
        self._ok("hipStreamSynchronize", stream)

    def device_sync(self):
        """hipDeviceSynchronize: for reference runs and clean-up, never inside a checked region"""
        self._ok("hipDeviceSynchronize")

    def busy(self, stream):
        """True while the stream holds unfinished work (hipStreamQuery says not-ready)"""
        rc = self.f["hipStreamQuery"](stream)
        self.f["hipGetLastError"]()            # (not-ready is an answer, not an error to leave behind for the next caller)
        assert rc in (HIP_SUCCESS, HIP_NOT_READY), "hipStreamQuery: HIP error %d" % rc
        return rc == HIP_NOT_READY

    def copy(self, dst, src, nbytes, stream):
        if nbytes:
            self._ok("hipMemcpyAsync", dst, src, nbytes, _D2D, stream)

    def fill(self, dst, byte, nbytes, stream):
        if nbytes:
            self._ok("hipMemsetAsync", dst, byte, nbytes, stream)

    # ---- events (to see whether two intervals overlapped) ----
    def event(self):
        e = _vp()
        self._ok("hipEventCreate", C.byref(e))
        return e.value

    def record(self, event, stream):
        self._ok("hipEventRecord", event, stream)

    def elapsed_ms(self, first, second):
        """milliseconds from one recorded event to another (negative: the second came first); both must have happened"""
        self._ok("hipEventSynchronize", first)
        self._ok("hipEventSynchronize", second)
        ms = C.c_float()
        self._ok("hipEventElapsedTime", C.byref(ms), first, second)
        return ms.value

    def event_destroy(self, event):
        self._ok("hipEventDestroy", event)


class Buf:
    """bytes of device memory from the library's allocator.  put / get are blocking copies on the null stream: for setting a case up and
    for reading it back after its streams have been synchronised, never inside the checked region"""

    def __init__(self, hip, init):
        """init: a number of bytes (left as allocated), or an array whose bytes the buffer starts with"""
        self.L = hip.L
        arr = None if isinstance(init, (int, np.integer)) else np.ascontiguousarray(init)
        self.nbytes = int(init) if arr is None else arr.nbytes
        self.ptr = self.L.fuifgpu_dev_alloc(max(self.nbytes, 16))
        assert self.ptr
        if arr is not None:
            self.put(arr)

    def put(self, arr):
        a = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        assert a.size <= self.nbytes
        if a.size:
            assert self.L.fuifgpu_dev_upload(self.ptr, a.ctypes.data, a.size) == 0
        return self

    def get(self, dtype=np.uint8, nbytes=None):
        out = np.empty(self.nbytes if nbytes is None else nbytes, np.uint8)
        if out.size:
            assert self.L.fuifgpu_dev_download(out.ctypes.data, self.ptr, out.size) == 0
        return out.view(dtype)

    def free(self):
        if self.ptr:
            self.L.fuifgpu_dev_free(self.ptr)
            self.ptr = None


class Gate:
    """A chain of large device-to-device copies between two scratch buffers: queued on a stream it keeps that stream busy for about the
    time asked for, and ends by itself -- nothing waits for the host, so a call under test that synchronised internally would merely
    wait the gate out.  The time of one copy is measured once, on a stream of its own, when the gate is made."""

    def __init__(self, hip, mib=256, probe=16):
        self.hip = hip
        self.nbytes = mib << 20
        self.a, self.b = Buf(hip, self.nbytes), Buf(hip, self.nbytes)
        s = hip.stream()
        try:
            hip.fill(self.a.ptr, 0, self.nbytes, s)
            hip.fill(self.b.ptr, 0, self.nbytes, s)
            self._chain(s, 4)                         # (the first copies pay for loading the copy kernel)
            hip.sync(s)
            t0 = time.perf_counter()
            self._chain(s, probe)
            hip.sync(s)
            self.copy_ms = (time.perf_counter() - t0) * 1e3 / probe
        finally:
            hip.destroy(s)

    def _chain(self, stream, copies):
        for k in range(copies):
            src, dst = (self.a, self.b) if k & 1 else (self.b, self.a)
            self.hip.copy(dst.ptr, src.ptr, self.nbytes, stream)

    def queue(self, stream, ms):
        """queue about `ms` milliseconds of copies on `stream` (None: the null stream); returns the number of copies"""
        copies = max(2, int(math.ceil(ms / self.copy_ms)))
        self._chain(stream, copies)
        return copies

    def free(self):
        self.a.free()
        self.b.free()
