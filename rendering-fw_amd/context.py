"""RenderContext over librfwhip.so — the HIP rendercore behind the reference's plugin interface
(RFW/system/context/rfw/context/context.h:74-111).  There is no CPU path: if the library or a HIP device is missing
the constructor raises."""
import ctypes as C
import os

from ._binding import CoreBinding, RenderGroup

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "librfwhip.so")
_lib = None


def load_library():
    """dlopen the in-tree librfwhip.so (RTLD_GLOBAL is not needed; HIP is linked in)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "librfwhip.so is missing (%s): build it with __graft_entry__.build(); "
                "the rendercore has no fallback path" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
    return _lib


class RenderContext(CoreBinding):
    def __init__(self, device=0, rank=0, world=1):
        super().__init__(load_library(), "rfwhip_", device, rank, world)


def render_group(devices, transport="auto"):
    """n devices of one node behind one object (rfwhip_group_*): RenderGroup over the in-tree librfwhip.so."""
    return RenderGroup(load_library(), "rfwhip_", devices, transport)


def comm_unique_id():
    """The 128-byte id rank 0 hands to the other ranks before rfwhip_comm_create (include/rfwhip.h)."""
    lib = load_library()
    buf = C.create_string_buffer(128)
    lib.rfwhip_comm_unique_id.restype, lib.rfwhip_comm_unique_id.argtypes = C.c_int, [C.c_void_p, C.c_size_t]
    if lib.rfwhip_comm_unique_id(buf, 128) != 0:
        lib.rfwhip_last_error.restype = C.c_char_p
        raise RuntimeError((lib.rfwhip_last_error() or b"unknown error").decode(errors="replace"))
    return buf.raw


class RenderComm:
    """One process per device: this rank's end of the strip gather (rfwhip_comm_*, RCCL issued by librfwhip.so).  Collective:
    every rank of the context's world constructs it with the same id, and every rank calls gather()."""

    def __init__(self, ctx, id_bytes):
        self._lib = load_library()
        vp, i32 = C.c_void_p, C.c_int
        for name, res, args in [("rfwhip_comm_create", i32, [vp, vp, C.POINTER(vp)]), ("rfwhip_comm_gather", i32, [vp, vp]),
                                ("rfwhip_comm_wait", i32, [vp]), ("rfwhip_comm_destroy", None, [vp]), ("rfwhip_last_error", C.c_char_p, [])]:
            f = getattr(self._lib, name)
            f.restype, f.argtypes = res, args
        self._c = vp()
        self._ctx = ctx
        self._id = C.create_string_buffer(bytes(id_bytes), 128) if id_bytes is not None else None
        self._check(self._lib.rfwhip_comm_create(ctx._ctx, self._id, C.byref(self._c)))

    def _check(self, code):
        if code != 0:
            raise RuntimeError((self._lib.rfwhip_last_error() or b"unknown error").decode(errors="replace"))

    def gather(self, full_rgba_device_ptr=0):
        """Enqueue present -> send / receive -> de-interleave (root: into the given device buffer, 0 = an internal one)."""
        self._check(self._lib.rfwhip_comm_gather(self._c, C.c_void_p(full_rgba_device_ptr or None)))

    def wait(self):
        self._check(self._lib.rfwhip_comm_wait(self._c))

    def display(self, full_rgba_device_ptr, out_device_ptr, format="rgba8", stream=0):
        """Root only: the display stage (rfwhip_display_stream) on the gathered full image, enqueued on the caller's
        hipStream_t (an int, e.g. torch.cuda.current_stream().cuda_stream; 0: the null stream) — order it behind the gather
        (wait(), or an event).  out: width * height * 4 bytes ("rgba8") or * 16 ("rgba32f") of device memory."""
        self._ctx.display_stream(full_rgba_device_ptr, out_device_ptr, format, stream)

    def display_jpeg(self, rgba8_device_ptr, out_device_ptr, cap, record_device_ptr, stream=0):
        """Root only: the JPEG encoder (rfwhip_display_jpeg_stream) on the RGBA8 image display() wrote, enqueued on the same
        stream behind it.  out: cap bytes of device memory (ctx.jpeg_bound() always suffices); record: 32 bytes whose first
        word is the stream's length once the stream has run."""
        self._ctx.display_jpeg_stream(rgba8_device_ptr, out_device_ptr, cap, record_device_ptr, stream)

    def destroy(self):
        if self._c:
            self._lib.rfwhip_comm_destroy(self._c)
            self._c = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
