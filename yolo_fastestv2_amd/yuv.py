"""Decoder-format frames: YUV 4:2:0 planes read in place (include/yfv2.h yfv2_frame_yuv).

    frame = YuvFrame((y, uv), "nv12", "bt709")                     # the two planes a video decoder wrote, as device tensors
    dets, idx, cnt = engine.detect_frames_yuv([frame, ...], 0.3, 0.4)
    crop = YuvFrame((y, uv), "nv12", "bt709", x0=101, y0=37, width=352, height=352)    # a rectangle of the same planes, no copy

``planes`` are uint8 device tensors: ``(y, uv)`` for NV12 / NV21 - uv either (rows, bytes) or (rows, samples, 2) - and
``(y, u, v)`` for I420 (YV12: pass ``(y, v, u)``).  A plane's row pitch is its ``stride(0)``; its bytes within a row must be
contiguous.  Nothing here needs a device; the table goes to libyfv2.so as it is.

The 10-bit formats have little-endian 16-bit samples: "p010" (semi-planar, the value in the high 10 bits: what
the hardware decoders write for HEVC Main10, AV1 and VP9 profile 2) and "i010" = "yuv420p10le" (planar, the value in the low 10
bits: what software decoders write).  Their planes are ``torch.int16`` tensors (``torch.uint16`` where this torch has it) of
shape (rows, samples) - uv also (rows, samples, 2) - with pitch ``2 * stride(0)``, or ``torch.uint8`` tensors holding the bytes,
with pitch ``stride(0)``.  A frame of byte tensors must state its ``width`` and ``height``: a byte plane is also a valid 8-bit
plane, so the rectangle is not guessed from it.  All frames of one call have one sample width.

The other 8-bit samplings - what a JPEG decoder writes for a file that is not 4:2:0, and what capture devices
deliver: "i444" = "yuv444p", "i422" = "yuv422p", "i440" = "yuv440p" take ``(y, u, v)``; "yuyv" = "yuy2" = "yuyv422", "uyvy" =
"uyvy422" and "grey" = "gray" = "y800" take ONE plane, ``(p,)`` or the tensor itself.  A packed plane is a 2-D uint8 tensor of
the bytes - two per pixel - or ``(rows, pixels, 2)``.  An alias picks the format only: the colour stays explicit ("jpeg" for
JPEG files).  One call may mix every 8-bit format; a call with a frame that is not 4:2:0 has the general launch's lower width
limit (``max_width(W, general=True)``) for all of its frames.
"""
import ctypes as C

import torch

from . import _lib

# What a format is, once: (YFV2_YUV_* code - bit 4: two-byte samples -, its name and pix_fmt aliases, bytes of a sample, planes - three: U
# and V in planes of their own -, chroma shifts (x, y), packed: one plane of 4-byte macropixels, two bytes per pixel; grey: luma only)
_TABLE = (
    (0, ("nv12",), 1, 2, (1, 1), False, False),
    (1, ("nv21",), 1, 2, (1, 1), False, False),
    (2, ("i420",), 1, 3, (1, 1), False, False),
    (3, ("i422", "yuv422p"), 1, 3, (1, 0), False, False),
    (4, ("i440", "yuv440p"), 1, 3, (0, 1), False, False),
    (5, ("i444", "yuv444p"), 1, 3, (0, 0), False, False),
    (6, ("yuyv", "yuy2", "yuyv422"), 1, 1, (1, 0), True, False),
    (7, ("uyvy", "uyvy422"), 1, 1, (1, 0), True, False),
    (8, ("grey", "gray", "y800"), 1, 1, (0, 0), False, True),
    (16, ("p010",), 2, 2, (1, 1), False, False),
    (17, ("i010", "yuv420p10le", "yuv420p10"), 2, 3, (1, 1), False, False),
)
FORMATS = {key: code for code, names, *_ in _TABLE for key in names + (code,)}
FORMAT_NAMES = {code: names[0] for code, names, *_ in _TABLE}
_SAMPLE_BYTES = {code: sb for code, _, sb, *_ in _TABLE}
sample_bytes = _SAMPLE_BYTES.__getitem__      # bytes of one sample of the (integer) format
_PLANES = {code: planes for code, _, _, planes, *_ in _TABLE}
SHIFTS = {code: shifts for code, _, _, _, shifts, *_ in _TABLE}      # format -> chroma shift (x, y)
PLANAR = tuple(code for code, planes in _PLANES.items() if planes == 3)
PACKED = tuple(row[0] for row in _TABLE if row[5])
GREY, = (row[0] for row in _TABLE if row[6])
WORD_DTYPES = tuple(getattr(torch, n) for n in ("int16", "uint16") if hasattr(torch, n))
COLOURS = {"bt601": 0, "bt601_limited": 0, "bt709": 1, "bt709_limited": 1, "bt601_full": 2, "jpeg": 2, "bt709_full": 3, 0: 0, 1: 1, 2: 2, 3: 3}
LDS_FULL = 160 * 1024
ROWS_U8, ROWS_COUNTED_U8, ROWS_TRAIN, ROWS_TENSOR_F32, ROWS_TENSOR_F16 = range(5)      # yfv2_debug_rows' row_kind


def _rows(hook, who, said, *args):      # the body of the three rows_lds*: `who(said)` is the caller, for the message
    lds, limit = C.c_int64(), C.c_int32()
    if getattr(_lib.lib(), hook)(*args, C.byref(lds), C.byref(limit)) != _lib.OK:
        raise ValueError("%s(%s): %s" % (who, ", ".join("%r" % (a,) for a in said), _lib.last_error()))
    return lds.value, limit.value


def rows_lds(kind, is_yuv, w, W):
    """(LDS bytes of one workgroup for a frame w pixels wide, the widest frame admitted) of the frame entry points' launch of row
    kind ``kind`` at output width W, as libyfv2.so itself computes them (include/yfv2.h yfv2_debug_rows; no device needed)"""
    return _rows("yfv2_debug_rows", "rows_lds", (kind, is_yuv, w, W), kind, int(bool(is_yuv)), w, W)


def resize_lds_bytes(w, W):
    """LDS of one workgroup of the YUV resize for a frame w pixels wide and an output row of W pixels: two luma slots, two chroma
    rows of two half-slots each, the output row."""
    return rows_lds(ROWS_U8, True, w, W)[0]


def rows_lds16(kind, w, W):
    """``rows_lds`` for YUV frames of two-byte samples ("p010", "i010"; include/yfv2.h yfv2_debug_rows16)"""
    return _rows("yfv2_debug_rows16", "rows_lds16", (kind, w, W), kind, w, W)


def rows_lds_any(kind, w, W):
    """``rows_lds`` for the general one-byte launch: a call with a frame that is not 4:2:0 (include/yfv2.h yfv2_debug_rows_any)"""
    return _rows("yfv2_debug_rows_any", "rows_lds_any", (kind, w, W), kind, w, W)


def max_width(W, bits=8, general=False):
    """the widest YUV frame the resize admits at network width W: bits = 8 for NV12 / NV21 / I420, 10 for P010 / I010;
    general=True: in a call with at least one 8-bit frame that is not 4:2:0 (which binds every frame of that call)"""
    if bits not in (8, 10):
        raise ValueError("bits must be 8 or 10, got %r" % (bits,))
    if general:
        if bits != 8:
            raise ValueError("the general launch reads 8-bit frames only")
        return rows_lds_any(ROWS_U8, 1, W)[1]
    return rows_lds(ROWS_U8, True, 1, W)[1] if bits == 8 else rows_lds16(ROWS_U8, 1, W)[1]


class YuvFrame:
    """One YUV frame: planes + format ("nv12", "nv21", "i420"; "p010", "i010" alias "yuv420p10le"; "i422", "i440", "i444", "yuyv",
    "uyvy", "grey" and their pix_fmt aliases) + colour ("bt601", "bt709" - limited range - "bt601_full" alias
    "jpeg", "bt709_full") and the rectangle of the planes that is the frame (default: all of the luma plane from (x0, y0) on; of a
    packed plane: all of its pixels, bytes // 2)."""
    __slots__ = ("planes", "format", "colour", "x0", "y0", "width", "height", "planar", "sample_bytes", "packed")

    def __init__(self, planes, format="nv12", colour="bt601", x0=0, y0=0, width=None, height=None):
        self.planes = (planes,) if torch.is_tensor(planes) else tuple(planes)
        if format not in FORMATS or isinstance(format, bool):
            raise ValueError("format must be one of 'nv12', 'nv21', 'i420', 'p010', 'i010' ('yuv420p10le'), 'i422', 'i440', 'i444', 'yuyv', 'uyvy', 'grey', got %r" % (format,))
        if colour not in COLOURS or isinstance(colour, bool):
            raise ValueError("colour must be one of 'bt601', 'bt709', 'bt601_full' ('jpeg'), 'bt709_full', got %r" % (colour,))
        self.format, self.colour = FORMATS[format], COLOURS[colour]
        self.planar, self.sample_bytes, self.packed = self.format in PLANAR, sample_bytes(self.format), self.format in PACKED
        self.x0, self.y0 = int(x0), int(y0)
        if self.packed:
            p = self.planes[0] if self.planes else None
            if not torch.is_tensor(p) or not (p.dim() == 2 or (p.dim() == 3 and p.shape[2] == 2)):
                raise ValueError("planes[0] must be the packed plane: 2-D bytes, or (rows, pixels, 2)")
            self.width = (int(p.shape[1]) // 2 if p.dim() == 2 else int(p.shape[1])) - self.x0 if width is None else int(width)
            self.height = int(p.shape[0]) - self.y0 if height is None else int(height)
            return
        if not self.planes or not torch.is_tensor(self.planes[0]) or self.planes[0].dim() != 2:
            raise ValueError("planes[0] must be the 2-D luma plane")
        if self.sample_bytes == 2 and self.planes[0].dtype == torch.uint8 and (width is None or height is None):
            raise ValueError("a %r frame of uint8 (byte) planes must state its width and height" % (format,))
        self.width = int(self.planes[0].shape[1]) - self.x0 if width is None else int(width)
        self.height = int(self.planes[0].shape[0]) - self.y0 if height is None else int(height)

    def crop(self, x0, y0, width, height):
        """the rectangle (x0, y0, width, height) of this frame as a frame of the same planes"""
        return YuvFrame(self.planes, self.format, self.colour, self.x0 + int(x0), self.y0 + int(y0), width, height)

    @property
    def shape(self):
        return (self.height, self.width)


def as_frame(f):
    """YuvFrame, or a bare tuple of planes: (y, uv) is NV12, (y, u, v) I420, both BT.601 limited range (every other format: a YuvFrame)"""
    if isinstance(f, YuvFrame):
        return f
    if isinstance(f, (tuple, list)) and len(f) in (2, 3) and all(torch.is_tensor(p) for p in f):
        return YuvFrame(f, "nv12" if len(f) == 2 else "i420")
    raise ValueError("expected a YuvFrame or a tuple of plane tensors (y, uv) / (y, u, v), got %s" % type(f).__name__)


# sample bytes -> (a plane's dtypes, their name, the unit of a row's length, the other shapes taken), for _plane's messages
_PLANE_WORDS = {1: ((torch.uint8,), "a uint8 tensor", "bytes", "uv may be (rows, samples, 2), a packed plane (rows, pixels, 2)"),
                2: (WORD_DTYPES, "an int16 / uint16 tensor (or uint8: the bytes)", "samples", "uv may be (rows, samples, 2)")}


def _plane(i, name, p, device, rows, row_samples, sb):
    """checks one plane against what the frame reads of it: `rows` rows of `row_samples` samples from its first one -> pitch in bytes.
    One-byte samples: a uint8 tensor.  Two-byte samples: a 16-bit tensor (pitch = 2 * stride(0)) or a uint8 tensor of the bytes
    (pitch = stride(0))."""
    if sb == 2 and torch.is_tensor(p) and p.dtype == torch.uint8:
        return _plane(i, name, p, device, rows, 2 * row_samples, 1)
    words = _PLANE_WORDS[sb]
    if not torch.is_tensor(p) or p.dtype not in words[0] or p.device != device:
        raise ValueError("frame %d: plane %s must be %s on %s" % (i, name, words[1], device))
    if p.dim() == 3 and p.shape[2] == 2 and name in ("uv", "packed") and (p.shape[1] <= 1 or p.stride(1) == 2) and p.stride(2) == 1:
        have = 2 * int(p.shape[1])
    elif p.dim() == 2 and (p.shape[1] <= 1 or p.stride(1) == 1):
        have = int(p.shape[1])
    else:
        raise ValueError("frame %d: plane %s must be 2-D with contiguous rows (%s)" % (i, name, words[3]))
    if p.shape[0] < rows or have < row_samples:
        raise ValueError("frame %d: plane %s is %d rows x %d %s, the frame reads %d x %d of it" % (i, name, p.shape[0], have, words[2], rows, row_samples))
    return sb * (int(p.stride(0)) if p.shape[0] > 1 else max(have, 1))


def frame_table(frames, device):
    """list / tuple of YuvFrame (or plane tuples) -> (yfv2_frame_yuv array, the frames).  Every plane must hold what its frame's
    rectangle reads: the native library sees pointers and pitches only and cannot check that."""
    if not isinstance(frames, (list, tuple)) or not frames or torch.is_tensor(frames[0]):
        raise ValueError("frames must be a non-empty list or tuple of YuvFrame")
    frames = [as_frame(f) for f in frames]
    arr = (_lib.FrameYuv * len(frames))()
    sb = frames[0].sample_bytes
    for i, f in enumerate(frames):
        planar = f.planar
        if f.sample_bytes != sb:
            raise ValueError("frame %d: %d-byte samples in a call whose frame 0 has %d-byte samples: one sample width per call" % (i, f.sample_bytes, sb))
        want = _PLANES[f.format]
        if len(f.planes) != want:
            raise ValueError("frame %d: %s takes %d plane%s, got %d" % (i, FORMAT_NAMES[f.format], want, "" if want == 1 else "s", len(f.planes)))
        if f.x0 < 0 or f.y0 < 0:
            raise ValueError("frame %d: x0 and y0 must be >= 0" % i)
        a = arr[i]
        a.x0, a.y0, a.width, a.height, a.format, a.colour = f.x0, f.y0, f.width, f.height, f.format, f.colour
        sx, sy = SHIFTS[f.format]
        if f.width >= 1 and f.height >= 1:      # (a frame without pixels is the native check's to report)
            crows, csamples = ((f.y0 + f.height - 1) >> sy) + 1, ((f.x0 + f.width - 1) >> sx) + 1
            if f.packed:                        # up to the last macropixel of the rectangle, whole
                a.pitch_y = _plane(i, "packed", f.planes[0], device, f.y0 + f.height, 4 * csamples, sb)
            else:
                a.pitch_y = _plane(i, "y", f.planes[0], device, f.y0 + f.height, f.x0 + f.width, sb)
            if planar:
                a.pitch_c = _plane(i, "u", f.planes[1], device, crows, csamples, sb)
                if _plane(i, "v", f.planes[2], device, crows, csamples, sb) != a.pitch_c:
                    raise ValueError("frame %d: planes u and v must have the same row pitch" % i)
                a.v = f.planes[2].data_ptr()
            elif want == 2:
                a.pitch_c = _plane(i, "uv", f.planes[1], device, crows, 2 * csamples, sb)
        a.y = f.planes[0].data_ptr()
        if want > 1:
            a.u = f.planes[1].data_ptr()
    return arr, frames
