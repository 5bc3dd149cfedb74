"""Every byte format of the project, host code only: ``bits_B.bin`` (the reference's), VCLD, VCIB, VCID, VCII, VCSQ, VCLI and VCLS (this
project's own; layout tables in INTEGRATION.md).  Nothing here touches a stream, a device tensor or a thread pool.

The formats share what they have in common and nothing else: :class:`Header` (bytes, short buffer, magic, version -- with the
format's label in every message), :func:`irans_payloads` (the length rule of the interleaved coder's payloads),
:func:`_icip2024_numbers` (the header fields VCIB and VCID share) and :func:`finish_all` (the deferred read of the device
decoders' error words).  Each format keeps its plain ``struct.Struct`` and its own field-range checks.  These headers size device
allocations: a reader validates everything before it returns anything (VcError)."""
import struct

import numpy as np

from . import hip
from .hip import VcError
from .lhbdc import check_container_shapes


class Header:
    """The fixed part of a format that opens with a 4-byte magic and a u8 version: ``layout`` is its whole struct.Struct, magic and
    version included.  ``unpack`` is how every reader starts, ``pack`` how every writer ends."""

    def __init__(self, label, magic, version, layout):
        self.label, self.magic, self.version, self.layout, self.size = label, magic, version, layout, layout.size

    def pack(self, *fields):
        return self.layout.pack(self.magic, self.version, *fields)

    def unpack(self, data):
        """(data as bytes, the fields behind magic and version); ``self.size`` bytes of ``data`` are the header."""
        data = bytes(data)
        if len(data) < self.size:
            raise VcError(f"{self.label}: {len(data)} bytes is shorter than the {self.size}-byte header")
        magic, version, *fields = self.layout.unpack_from(data, 0)
        if magic != self.magic:
            raise VcError(f"{self.label}: magic {magic!r} is not {self.magic!r}")
        if version != self.version:
            raise VcError(f"{self.label}: version {version} (this reader knows {self.version})")
        return data, fields


def _split(data, pos, lengths):
    parts = []
    for n in lengths:
        parts.append(data[pos:pos + n])
        pos += n
    return parts


def irans_payloads(label, waves, lengths, fixed, data):
    """The payloads of the interleaved coder (include/vc_hip.h: "Interleaved range coder") that lie back to back behind the ``fixed``
    header bytes of ``data``: a valid wave count, lengths that account for every byte (no trailing ones), whole 32-bit words, and
    at least the W sub-stream headers in each -- or VcError."""
    if not hip.irans_waves_ok(waves):
        raise VcError(f"{label}: waves {waves} is not a power of two in 1..16")
    if fixed + sum(lengths) != len(data) or any(n % 4 or n < waves * hip.IRANS_SUBSTREAM_HEADER for n in lengths):
        raise VcError(f"{label}: payload lengths {' + '.join(str(n) for n in lengths)} do not fit {len(data)} bytes / {waves} waves")
    return _split(data, fixed, lengths)


def finish_all(decoders):
    """``finish()`` of every item (hip.IransDecoder, or anything that holds some): the one read of each decoder's error words.  Every
    one is read before the first VcError is raised."""
    errors = []
    for d in decoders:
        try:
            d.finish()
        except VcError as e:
            errors.append(e)
    if errors:
        raise errors[0]


def _fits_u32(what, blobs):
    if any(len(b) > 0xffffffff for b in blobs):
        raise VcError(f"{what} is longer than the container's 32-bit length field")


# ------------------------------------------------------------------------------------------------
# bits_B.bin: the reference's container of one LHBDC B-frame (encode_B.py:114-126; the reader is lhbdc.read_container)
# ------------------------------------------------------------------------------------------------
# u32 lambda | u16 x 2 mv z-shape | u32 len(mv_y) | u32 len(mv_z) | u16 x 2 res z-shape | u32 len(res_y) | mv_y | mv_z | res_y | res_z
# (to the end of the file); little-endian, no magic.
BITS_B_HEADER = struct.Struct("<IHHIIHHI")


def pack_bits_b(lmbda, mv_shape, res_shape, mv_y, mv_z, res_y, res_z):
    mh, mw, rh, rw = (int(v) for v in tuple(mv_shape) + tuple(res_shape))
    return b"".join((BITS_B_HEADER.pack(int(lmbda), mh, mw, len(mv_y), len(mv_z), rh, rw, len(res_y)), mv_y, mv_z, res_y, res_z))


# ------------------------------------------------------------------------------------------------
# Device-coded LHBDC B-frame container (this project's own format; bits_B.bin stays the default and the reference's)
# ------------------------------------------------------------------------------------------------
# One byte string per coded frame, little-endian:
#   offset  0  4 bytes  magic "VCLD"
#           4  u8       version (1)
#           5  u8       waves W (1, 2, 4, 8 or 16): sub-streams per payload
#           6  u32      lambda (as bits_B.bin)
#          10  u16 x 2  hyper-latent shape (h, w) of the motion compressor
#          14  u16 x 2  hyper-latent shape (h, w) of the residual compressor
#          18  u32 x 2  payload lengths: motion, residual
#          26  the two payloads in that order
# A payload is one interleaved-rANS payload (include/vc_hip.h: "Interleaved range coder") of two segments, states and cursors
# continuing from the first to the second: the hyper-latent z (table set 0 = the factorised tables, index of symbol i =
# i / (hz * wz), its channel), then the latent y (table set 1 = the Gaussian tables, index from the scales); symbol order = the int32
# tensors of MeanScaleHyperprior.code_t (NCHW raster).
LHBDC_DEV_MAGIC = b"VCLD"
LHBDC_DEV_VERSION = 1
LHBDC_DEV_HEADER = struct.Struct("<4sBBIHHHHII")
_VCLD = Header("VCLD container", LHBDC_DEV_MAGIC, LHBDC_DEV_VERSION, LHBDC_DEV_HEADER)


def pack_lhbdc_frame_dev(lmbda, mv_shape, res_shape, waves, mv_payload, res_payload):
    """The VCLD container of one frame from the two payloads of ``LhbdcStreamCodec(coder="device")``."""
    shapes = tuple(int(v) for v in tuple(mv_shape) + tuple(res_shape))
    if len(shapes) != 4 or not all(1 <= v <= 0xffff for v in shapes) or not hip.irans_waves_ok(waves) or not 0 <= int(lmbda) <= 0xffffffff:
        raise VcError(f"lambda {lmbda} / hyper-latent shapes {shapes} / waves {waves} do not fit the container")
    mv_payload, res_payload = bytes(mv_payload), bytes(res_payload)
    _fits_u32("a payload", (mv_payload, res_payload))
    return _VCLD.pack(int(waves), int(lmbda), *shapes, len(mv_payload), len(res_payload)) + mv_payload + res_payload


def unpack_lhbdc_frame_dev(data, h, w):
    """Inverse of :func:`pack_lhbdc_frame_dev` for a (padded) h x w frame: ``{"lmbda", "waves", "mv_shape", "res_shape", "mv", "res"}``.
    Magic, version, wave count, the lengths against the data (no trailing bytes, whole words, at least the W sub-stream headers)
    and the shapes against the frame size (lhbdc.check_container_shapes) are validated before anything is returned, so before
    anything is allocated from the header (VcError)."""
    data, (waves, lmbda, mh, mw, rh, rw, n_mv, n_res) = _VCLD.unpack(data)
    mv, res = irans_payloads(_VCLD.label, waves, (n_mv, n_res), _VCLD.size, data)
    check_container_shapes((mh, mw), (rh, rw), h, w)
    return {"lmbda": lmbda, "waves": waves, "mv_shape": (mh, mw), "res_shape": (rh, rw), "mv": mv, "res": res}


# ------------------------------------------------------------------------------------------------
# ICIP2024 B-frame container (this project's own format: the reference has no bitstream for FlowGuidedB)
# ------------------------------------------------------------------------------------------------
# One byte string per coded frame, little-endian:
#   offset  0  4 bytes  magic "VCIB"
#           4  u8       version (1)
#           5  u8       down_ratio (1, 2, 4, 8 or 16)
#           6  u16 x 2  hyper-latent shape (h, w) = frame / 64
#          10  f32 x 3  s (quality level), scale1, scale2 (both after FlowGuidedB.convert_scales)
#          22  u32 x 12 string lengths: offset z, offset g0..g4, residual z, residual g0..g4
#          70  the twelve payloads in that order
ICIP2024_MAGIC = b"VCIB"
ICIP2024_VERSION = 1
ICIP2024_HEADER = struct.Struct("<4sBBHHfff")
ICIP2024_LENGTHS = struct.Struct("<12I")
ICIP2024_DOWN_RATIOS = (1, 2, 4, 8, 16)
_VCIB = Header("ICIP2024 container", ICIP2024_MAGIC, ICIP2024_VERSION, struct.Struct(ICIP2024_HEADER.format + "12I"))


def _icip2024_numbers(label, down_ratio, hz, wz, s, scale1, scale2):
    """The 18 header bytes behind magic and version that VCIB and VCID share, as both writers store and both readers return them --
    or VcError."""
    down_ratio, hz, wz = int(down_ratio), int(hz), int(wz)
    if down_ratio not in ICIP2024_DOWN_RATIOS or not (1 <= hz <= 0xffff and 1 <= wz <= 0xffff):
        raise VcError(f"{label}: down_ratio {down_ratio} / hyper-latent shape {hz}x{wz} out of range")
    s, scale1, scale2 = float(s), float(scale1), float(scale2)
    if not all(np.isfinite(v) for v in (s, scale1, scale2)):
        raise VcError(f"{label}: a header number is not finite")
    return down_ratio, hz, wz, s, scale1, scale2


def _icip2024_payloads(strings, image):
    out = []
    for codec in ("offset", "residual"):
        groups, z = strings[codec]
        if len(groups) != 5:
            raise VcError(f"{codec}: five group strings per image, got {len(groups)}")
        out.append(z[image])
        out.extend(g[image] for g in groups)
    return [bytes(b) for b in out]


def pack_icip2024_frame(strings, shape, down_ratio, s, scale1, scale2, image=0):
    """The container of image ``image`` of a FlowGuidedB.compress result: ``strings`` / ``shape`` / ``down_ratio`` as it returns
    them, ``s`` the quality level and ``scale1`` / ``scale2`` the converted scales (FlowGuidedB.convert_scales) it was called
    with.  The three numbers are stored as fp32 -- compress() and decompress() round the level to fp32 themselves and the
    converted scales are fp32 values, so a decoder fed from the container uses the encoder's numbers."""
    numbers = _icip2024_numbers(_VCIB.label, down_ratio, shape[0], shape[1], s, scale1, scale2)
    payloads = _icip2024_payloads(strings, image)
    _fits_u32("a string", payloads)
    return _VCIB.pack(*numbers, *(len(p) for p in payloads)) + b"".join(payloads)


def unpack_icip2024_frame(data):
    """Inverse of :func:`pack_icip2024_frame`: ``{"strings" (one image per list), "shape", "down_ratio", "s", "scale1", "scale2"}``.
    Magic, version, field ranges and the total length are validated before anything is returned (VcError)."""
    data, fields = _VCIB.unpack(data)
    down_ratio, hz, wz, s, scale1, scale2 = _icip2024_numbers(_VCIB.label, *fields[:6])
    lengths = fields[6:]
    if _VCIB.size + sum(lengths) != len(data):
        raise VcError(f"{_VCIB.label}: the length table asks for {_VCIB.size + sum(lengths)} bytes, the buffer has {len(data)}")
    parts = _split(data, _VCIB.size, lengths)
    strings = {"offset": [[[p] for p in parts[1:6]], [parts[0]]], "residual": [[[p] for p in parts[7:12]], [parts[6]]]}
    return {"strings": strings, "shape": (hz, wz), "down_ratio": down_ratio, "s": s, "scale1": scale1, "scale2": scale2}


# Container of the device-coded frames (FlowGuidedB.compress(coder="device"); payload format: DESIGN.md section 4d).  Its own
# magic: a VCIB reader refuses it and this reader refuses VCIB.  Little-endian:
#   offset  0  the 22 header bytes of VCIB with magic "VCID": version (1), down_ratio, hyper-latent shape, s, scale1, scale2
#          22  u8       waves W (1, 2, 4, 8 or 16): sub-streams per payload
#          23  u32 x 2  payload lengths: offset, residual
#          31  the two payloads in that order
ICIP2024_DEV_MAGIC = b"VCID"
ICIP2024_DEV_TAIL = struct.Struct("<BII")
_VCID = Header("ICIP2024 device-coded container", ICIP2024_DEV_MAGIC, ICIP2024_VERSION, struct.Struct(ICIP2024_HEADER.format + "BII"))


def pack_icip2024_frame_dev(strings, shape, down_ratio, s, scale1, scale2, waves, image=0):
    """The container of image ``image`` of a ``FlowGuidedB.compress(coder="device")`` result (``waves`` as it returns it)."""
    numbers = _icip2024_numbers(_VCID.label, down_ratio, shape[0], shape[1], s, scale1, scale2)
    if not hip.irans_waves_ok(waves):
        raise VcError(f"{_VCID.label}: waves {waves} is not a power of two in 1..16")
    if not isinstance(strings, dict) or set(strings) != {"offset", "residual"}:
        raise VcError('strings: {"offset": [payload per image], "residual": [payload per image]}')
    payloads = [bytes(strings[c][image]) for c in ("offset", "residual")]
    _fits_u32("a payload", payloads)
    return _VCID.pack(*numbers, int(waves), *(len(p) for p in payloads)) + b"".join(payloads)


def unpack_icip2024_frame_dev(data):
    """Inverse of :func:`pack_icip2024_frame_dev`: ``{"strings" (one image per list), "waves", "shape", "down_ratio", "s", "scale1",
    "scale2"}``; magic, version, field ranges, the wave count, the smallest possible payload and the total length are validated
    before anything is returned (VcError)."""
    data, (*numbers, waves, n_off, n_res) = _VCID.unpack(data)
    down_ratio, hz, wz, s, scale1, scale2 = _icip2024_numbers(_VCID.label, *numbers)
    offset, residual = irans_payloads(_VCID.label, waves, (n_off, n_res), _VCID.size, data)
    strings = {"offset": [offset], "residual": [residual]}
    return {"strings": strings, "waves": waves, "shape": (hz, wz), "down_ratio": down_ratio, "s": s, "scale1": scale1, "scale2": scale2}


# ------------------------------------------------------------------------------------------------
# ICIP2024 sequence file: device-coded ELIC I-frames (VCII) and B-frames (VCID) in coding order (VCSQ).  Layout: INTEGRATION.md
# ------------------------------------------------------------------------------------------------
# I-frame container, little-endian:
#   offset  0  4 bytes  magic "VCII"
#           4  u8       version (1)
#           5  u8       waves W (1, 2, 4, 8 or 16)
#           6  u16 x 2  hyper-latent shape (h, w) = frame / 64
#          10  u32      payload length
#          14  the payload of ELIC.compress(coder="device") for one image
ICIP2024_INTRA_MAGIC = b"VCII"
ICIP2024_INTRA_VERSION = 1
ICIP2024_INTRA_HEADER = struct.Struct("<4sBBHHI")
_VCII = Header("ICIP2024 I-frame container", ICIP2024_INTRA_MAGIC, ICIP2024_INTRA_VERSION, ICIP2024_INTRA_HEADER)


def pack_icip2024_intra_dev(payload, shape, waves):
    """The container of one image of an ``ELIC.compress(coder="device")`` result: its payload, "shape" and "waves"."""
    hz, wz = int(shape[0]), int(shape[1])
    payload = bytes(payload)
    if not (1 <= hz <= 0xffff and 1 <= wz <= 0xffff):
        raise VcError(f"hyper-latent shape {hz}x{wz} does not fit the container")
    _fits_u32("a payload", (payload,))
    irans_payloads(_VCII.label, waves, (len(payload),), 0, payload)
    return _VCII.pack(int(waves), hz, wz, len(payload)) + payload


def unpack_icip2024_intra_dev(data):
    """Inverse of :func:`pack_icip2024_intra_dev`: ``{"payload", "waves", "shape"}``; magic, version, the wave count, the smallest
    possible payload and the total length are validated before anything is returned (VcError)."""
    data, (waves, hz, wz, length) = _VCII.unpack(data)
    if hz < 1 or wz < 1:
        raise VcError(f"{_VCII.label}: hyper-latent shape {hz}x{wz} out of range")
    (payload,) = irans_payloads(_VCII.label, waves, (length,), _VCII.size, data)
    return {"payload": payload, "waves": waves, "shape": (hz, wz)}


# Sequence file, little-endian:
#   offset  0  4 bytes  magic "VCSQ"
#           4  u8       version (1)
#           5  u8       model family (1 = ICIP2024; every other value is refused)
#           6  u16 x 2  picture width, height (unpadded)
#          10  u32      frame count
#          14  u16      intra_size
#          16  f32      quality level s
#          20  u8       intra quality index
#          21  one record per frame in CODING order:  u8 type (0 = I, 1 = B) | u32 display order | u32 length | VCII / VCID bytes
SEQUENCE_MAGIC = b"VCSQ"
SEQUENCE_VERSION = 1
SEQUENCE_FAMILY_ICIP2024 = 1
SEQUENCE_HEADER = struct.Struct("<4sBBHHIHfB")
SEQUENCE_RECORD = struct.Struct("<BII")
SEQUENCE_TYPES = ("I", "B")
_VCSQ = Header("sequence file", SEQUENCE_MAGIC, SEQUENCE_VERSION, SEQUENCE_HEADER)


def sequence_plan(intra_size, n_frames):
    """[(display order, "I" | "B")] in coding order, as the encoder's loop walks it (icip2024.get_order_typ_list).  VcError where
    that function gives no coding order for the pair: every frame exactly once, the first one an I-frame."""
    from . import icip2024
    intra_size, n_frames = int(intra_size), int(n_frames)
    if intra_size < 1 or n_frames < 1:
        raise VcError(f"intra_size {intra_size} / {n_frames} frames: both at least 1")
    if n_frames == 1:
        return [(0, "I")]
    order, typ = icip2024.get_order_typ_list(intra_size, n_frames)
    if sorted(order) != list(range(n_frames)) or len(typ) != n_frames or typ[order[0]] != "I":
        raise VcError(f"get_order_typ_list({intra_size}, {n_frames}) is no coding order of {n_frames} frames: {order}")
    return [(o, typ[o]) for o in order]


def pack_sequence(records, width, height, intra_size, s, intra_quality, family=SEQUENCE_FAMILY_ICIP2024):
    """``records``: [(type "I" | "B", display order, container bytes)] in coding order -- checked against :func:`sequence_plan`."""
    records = [(t, int(o), bytes(b)) for t, o, b in records]
    if family != SEQUENCE_FAMILY_ICIP2024:
        raise VcError(f"sequence file: model family {family} (only {SEQUENCE_FAMILY_ICIP2024} = ICIP2024 is defined)")
    if not (1 <= int(width) <= 0xffff and 1 <= int(height) <= 0xffff and 1 <= int(intra_size) <= 0xffff and 0 <= int(intra_quality) <= 0xff) \
            or not np.isfinite(float(s)) or not 1 <= len(records) <= 0xffffffff:
        raise VcError("sequence file: a header field is out of range")
    if [(o, t) for t, o, _ in records] != sequence_plan(intra_size, len(records)):
        raise VcError("sequence file: the records are not in the coding order of get_order_typ_list")
    if any(len(b) > 0xffffffff for _, _, b in records):
        raise VcError("sequence file: a frame is longer than the 32-bit length field")
    head = _VCSQ.pack(family, int(width), int(height), len(records), int(intra_size), float(s), int(intra_quality))
    return head + b"".join(SEQUENCE_RECORD.pack(SEQUENCE_TYPES.index(t), o, len(b)) + b for t, o, b in records)


def unpack_sequence(data):
    """Inverse of :func:`pack_sequence`: ``{"family", "width", "height", "frames", "intra_size", "s", "intra_quality", "records":
    [(type, display order, container bytes)] in coding order}``.  Magic, version, family, field ranges, the frame count against the
    buffer's length (before anything is sized by it), every record's length against the data that is left, the record sequence
    against :func:`sequence_plan` and the absence of trailing bytes are validated before anything is returned (VcError)."""
    data, (family, width, height, frames, intra_size, s, intra_quality) = _VCSQ.unpack(data)
    if family != SEQUENCE_FAMILY_ICIP2024:
        raise VcError(f"sequence file: model family {family} (only {SEQUENCE_FAMILY_ICIP2024} = ICIP2024 is defined)")
    if width < 1 or height < 1 or intra_size < 1 or not np.isfinite(s):
        raise VcError(f"sequence file: picture {width}x{height} / intra_size {intra_size} / level {s} out of range")
    if frames < 1 or _VCSQ.size + frames * SEQUENCE_RECORD.size > len(data):
        raise VcError(f"sequence file: {frames} frames do not fit {len(data)} bytes")
    plan = sequence_plan(intra_size, frames)
    records, pos = [], _VCSQ.size
    for k, (order, typ) in enumerate(plan):
        if pos + SEQUENCE_RECORD.size > len(data):
            raise VcError(f"sequence file: the data ends before record {k} of {frames}")
        t, o, length = SEQUENCE_RECORD.unpack_from(data, pos)
        pos += SEQUENCE_RECORD.size
        if t >= len(SEQUENCE_TYPES) or (o, SEQUENCE_TYPES[t]) != (order, typ):
            raise VcError(f"sequence file: record {k} is (order {o}, type {t}), the coding order asks for ({order}, {typ})")
        if length > len(data) - pos:
            raise VcError(f"sequence file: record {k} asks for {length} bytes, {len(data) - pos} are left")
        records.append((typ, o, data[pos:pos + length]))
        pos += length
    if pos != len(data):
        raise VcError(f"sequence file: {len(data) - pos} trailing bytes behind the last record")
    return {"family": family, "width": width, "height": height, "frames": frames, "intra_size": intra_size, "s": s,
            "intra_quality": intra_quality, "records": records}


# ------------------------------------------------------------------------------------------------
# LHBDC sequence file: device-coded mbt2018_mean I-frames (VCLI) and B-frames (VCLD) in coding order (VCLS).  Layout: INTEGRATION.md
# ------------------------------------------------------------------------------------------------
# I-frame container, little-endian:
#   offset  0  4 bytes  magic "VCLI"
#           4  u8       version (1)
#           5  u8       waves W (1, 2, 4, 8 or 16)
#           6  u16 x 2  hyper-latent shape (h, w) = frame / 64
#          10  u32      payload length
#          14  the payload of ImageMeanScaleHyperprior.compress(coder="device") for one image (two segments, as a VCLD payload)
LHBDC_INTRA_MAGIC = b"VCLI"
LHBDC_INTRA_VERSION = 1
LHBDC_INTRA_HEADER = struct.Struct("<4sBBHHI")
_VCLI = Header("LHBDC I-frame container", LHBDC_INTRA_MAGIC, LHBDC_INTRA_VERSION, LHBDC_INTRA_HEADER)


def pack_lhbdc_intra_dev(payload, shape, waves):
    """The container of one image of an ``ImageMeanScaleHyperprior.compress(coder="device")`` result: its payload, "shape" and
    "waves"."""
    hz, wz = int(shape[0]), int(shape[1])
    payload = bytes(payload)
    if not (1 <= hz <= 0xffff and 1 <= wz <= 0xffff):
        raise VcError(f"hyper-latent shape {hz}x{wz} does not fit the container")
    _fits_u32("a payload", (payload,))
    irans_payloads(_VCLI.label, waves, (len(payload),), 0, payload)
    return _VCLI.pack(int(waves), hz, wz, len(payload)) + payload


def unpack_lhbdc_intra_dev(data):
    """Inverse of :func:`pack_lhbdc_intra_dev`: ``{"payload", "waves", "shape"}``; magic, version, the wave count, the smallest
    possible payload and the total length are validated before anything is returned (VcError)."""
    data, (waves, hz, wz, length) = _VCLI.unpack(data)
    if hz < 1 or wz < 1:
        raise VcError(f"{_VCLI.label}: hyper-latent shape {hz}x{wz} out of range")
    (payload,) = irans_payloads(_VCLI.label, waves, (length,), _VCLI.size, data)
    return {"payload": payload, "waves": waves, "shape": (hz, wz)}


# Sequence file, little-endian:
#   offset  0  4 bytes  magic "VCLS"
#           4  u8       version (1)
#           5  u8       flags: bit 0 = every record carries the hash of its decoded picture; every other bit is refused
#           6  u16 x 2  picture width, height (unpadded)
#          10  u32      frame count N
#          14  u32      lambda (as bits_B.bin and VCLD)
#          18  u8       intra quality (1..8: the mbt2018_mean quality of the I-frames)
#          19  one record per frame in CODING order:
#                u8 type (0 = I, 1 = B) | u32 display order | u32 length | u64 picture hash (only with flag bit 0) | VCLI / VCLD bytes
LHBDC_SEQUENCE_MAGIC = b"VCLS"
LHBDC_SEQUENCE_VERSION = 1
LHBDC_SEQUENCE_HASHES = 1                # flag bit 0
LHBDC_SEQUENCE_HEADER = struct.Struct("<4sBBHHIIB")
LHBDC_SEQUENCE_RECORD = struct.Struct("<BII")
LHBDC_SEQUENCE_HASH = struct.Struct("<Q")
LHBDC_GOP = 8
_VCLS = Header("LHBDC sequence file", LHBDC_SEQUENCE_MAGIC, LHBDC_SEQUENCE_VERSION, LHBDC_SEQUENCE_HEADER)


def lhbdc_sequence_plan(n_frames):
    """[(display order, "I" | "B")] in coding order for N frames: I(0); for each of the (N - 1) // 8 whole GOPs its closing I-frame
    8k + 8, then its seven B-frames in hierarchy order (gop.LEVEL_GROUPS: 4; 2, 6; 1, 3, 5, 7); then the (N - 1) % 8 frames behind
    the last whole GOP as I-frames in display order.  A boundary I-frame is listed (and coded) once."""
    from .gop import LEVEL_GROUPS
    n_frames = int(n_frames)
    if n_frames < 1:
        raise VcError(f"{n_frames} frames: at least 1")
    gops = (n_frames - 1) // LHBDC_GOP
    plan = [(0, "I")]
    for k in range(gops):
        plan.append((LHBDC_GOP * k + LHBDC_GOP, "I"))
        plan.extend((LHBDC_GOP * k + o, "B") for group in LEVEL_GROUPS for o in group)
    plan.extend((o, "I") for o in range(LHBDC_GOP * gops + 1, n_frames))
    return plan


def _lhbdc_sequence_numbers(width, height, lmbda, intra_quality):
    width, height, lmbda, intra_quality = int(width), int(height), int(lmbda), int(intra_quality)
    if not (1 <= width <= 0xffff and 1 <= height <= 0xffff and 0 <= lmbda <= 0xffffffff and 1 <= intra_quality <= 8):
        raise VcError(f"{_VCLS.label}: picture {width}x{height} / lambda {lmbda} / intra quality {intra_quality} (1..8) out of range")
    return width, height, lmbda, intra_quality


def pack_lhbdc_sequence(records, width, height, lmbda, intra_quality, hashes=None):
    """``records``: [(type "I" | "B", display order, container bytes)] in coding order -- checked against
    :func:`lhbdc_sequence_plan`.  ``hashes``: {display order: uint64 hash of the decoded picture} for every frame, or None for a
    file without hashes (flag bit 0 clear)."""
    records = [(t, int(o), bytes(b)) for t, o, b in records]
    width, height, lmbda, intra_quality = _lhbdc_sequence_numbers(width, height, lmbda, intra_quality)
    if not 1 <= len(records) <= 0xffffffff:
        raise VcError(f"{_VCLS.label}: {len(records)} frames do not fit the header")
    if [(o, t) for t, o, _ in records] != lhbdc_sequence_plan(len(records)):
        raise VcError(f"{_VCLS.label}: the records are not in the coding order of lhbdc_sequence_plan")
    _fits_u32("a frame", [b for _, _, b in records])
    if hashes is not None and (sorted(hashes) != list(range(len(records))) or not all(0 <= int(v) <= 0xffffffffffffffff for v in hashes.values())):
        raise VcError(f"{_VCLS.label}: one 64-bit picture hash per frame")
    flags = 0 if hashes is None else LHBDC_SEQUENCE_HASHES
    parts = [_VCLS.pack(flags, width, height, len(records), lmbda, intra_quality)]
    for t, o, b in records:
        parts.append(LHBDC_SEQUENCE_RECORD.pack(SEQUENCE_TYPES.index(t), o, len(b)))
        if hashes is not None:
            parts.append(LHBDC_SEQUENCE_HASH.pack(int(hashes[o])))
        parts.append(b)
    return b"".join(parts)


def unpack_lhbdc_sequence(data):
    """Inverse of :func:`pack_lhbdc_sequence`: ``{"flags", "width", "height", "frames", "lmbda", "intra_quality", "records": [(type,
    display order, container bytes)] in coding order, "hashes": {display order: int} or None}``.  Magic, version, flags, field
    ranges, the frame count against the buffer's length (before anything is sized by it), every record's type and order against
    :func:`lhbdc_sequence_plan`, every length against the data that is left and the absence of trailing bytes are validated
    before anything is returned (VcError)."""
    data, (flags, width, height, frames, lmbda, intra_quality) = _VCLS.unpack(data)
    if flags & ~LHBDC_SEQUENCE_HASHES:
        raise VcError(f"{_VCLS.label}: flags {flags:#04x} (only bit 0, picture hashes, is defined)")
    _lhbdc_sequence_numbers(width, height, lmbda, intra_quality)
    fixed = LHBDC_SEQUENCE_RECORD.size + (LHBDC_SEQUENCE_HASH.size if flags & LHBDC_SEQUENCE_HASHES else 0)
    if frames < 1 or _VCLS.size + frames * fixed > len(data):
        raise VcError(f"{_VCLS.label}: {frames} frames do not fit {len(data)} bytes")
    plan = lhbdc_sequence_plan(frames)
    records, hashes, pos = [], ({} if flags & LHBDC_SEQUENCE_HASHES else None), _VCLS.size
    for k, (order, typ) in enumerate(plan):
        if pos + fixed > len(data):
            raise VcError(f"{_VCLS.label}: the data ends before record {k} of {frames}")
        t, o, length = LHBDC_SEQUENCE_RECORD.unpack_from(data, pos)
        if t >= len(SEQUENCE_TYPES) or (o, SEQUENCE_TYPES[t]) != (order, typ):
            raise VcError(f"{_VCLS.label}: record {k} is (order {o}, type {t}), the coding order asks for ({order}, {typ})")
        if hashes is not None:
            (hashes[o],) = LHBDC_SEQUENCE_HASH.unpack_from(data, pos + LHBDC_SEQUENCE_RECORD.size)
        pos += fixed
        if length > len(data) - pos:
            raise VcError(f"{_VCLS.label}: record {k} asks for {length} bytes, {len(data) - pos} are left")
        records.append((typ, o, data[pos:pos + length]))
        pos += length
    if pos != len(data):
        raise VcError(f"{_VCLS.label}: {len(data) - pos} trailing bytes behind the last record")
    return {"flags": flags, "width": width, "height": height, "frames": frames, "lmbda": lmbda, "intra_quality": intra_quality,
            "records": records, "hashes": hashes}
