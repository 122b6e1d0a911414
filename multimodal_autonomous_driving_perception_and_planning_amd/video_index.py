"""Where the frames lie in a Motion-JPEG file: host logic only, importable without a device.

index_avi(buf)    RIFF AVI 1.0 with an MJPG video stream -> {"width", "height", "fps", "frames": [(offset, length)], "indexed"}
index_mjpeg(buf)  a raw concatenation of JPEG frames      -> [(offset, length)]
jpeg_size(buf, offset, length)  -> (width, height) of the frame header, or None
AviWriter(path, fps, width, height)  writes such an AVI: add(jpeg_bytes) per frame, close() patches the counts and appends idx1

`buf` is anything with len(), slicing to bytes and find(): bytes, or an mmap of the file.  Every (offset, length) lies inside buf.
"""
import struct


def _u32(buf, pos):
    """Little-endian dword at pos; a file that ends inside it is a ValueError, like everything else that is wrong with a file."""
    if pos < 0 or pos + 4 > len(buf):
        raise ValueError("truncated AVI: a header field at offset %d lies behind the end of the file" % pos)
    return struct.unpack_from("<I", buf[pos:pos + 4])[0]


def _i32(buf, pos):
    v = _u32(buf, pos)
    return v - (1 << 32) if v & 0x80000000 else v


def index_avi(buf):
    n = len(buf)
    if n < 12 or buf[0:4] != b"RIFF" or buf[8:12] != b"AVI ":
        raise ValueError("not a RIFF AVI file")
    info = {"width": 0, "height": 0, "fps": 0.0, "frames": [], "indexed": False}
    usec, n_streams, vid, handler, comp, scale, rate = 0, 0, None, b"", b"", 0, 0
    movi = idx1 = None
    pos = 12
    while pos + 8 <= n:
        cc, size = buf[pos:pos + 4], _u32(buf, pos + 4)
        end = min(pos + 8 + size, n)
        if cc == b"LIST" and buf[pos + 8:pos + 12] == b"hdrl":
            p = pos + 12
            while p + 8 <= end:
                c2, s2 = buf[p:p + 4], _u32(buf, p + 4)
                if c2 == b"avih" and s2 >= 40:
                    usec = _u32(buf, p + 8)
                    info["width"], info["height"] = _u32(buf, p + 8 + 32), _u32(buf, p + 8 + 36)
                elif c2 == b"LIST" and buf[p + 8:p + 12] == b"strl":
                    q, e2, is_vid = p + 12, min(p + 8 + s2, end), False
                    while q + 8 <= e2:
                        c3, s3 = buf[q:q + 4], _u32(buf, q + 4)
                        if c3 == b"strh" and s3 >= 32:
                            is_vid = buf[q + 8:q + 12] == b"vids" and vid is None
                            if is_vid:
                                vid, handler = n_streams, buf[q + 12:q + 16]
                                scale, rate = _u32(buf, q + 8 + 20), _u32(buf, q + 8 + 24)
                        elif c3 == b"strf" and is_vid and s3 >= 20:
                            comp = buf[q + 8 + 16:q + 8 + 20]
                            w, h = _i32(buf, q + 12), _i32(buf, q + 16)
                            if w > 0 and h != 0:
                                info["width"], info["height"] = w, abs(h)
                        elif c3 == b"indx" and is_vid:
                            raise ValueError("OpenDML AVI (a super-index 'indx' chunk) is not supported")
                        q += 8 + s3 + (s3 & 1)
                    n_streams += 1
                p += 8 + s2 + (s2 & 1)
        elif cc == b"LIST" and buf[pos + 8:pos + 12] == b"movi" and movi is None:
            movi = (pos + 8, end)                      # from the 'movi' tag to the end of the list
        elif cc == b"idx1":
            idx1 = (pos + 8, end)
        pos += 8 + size + (size & 1)                    # JUNK and anything else: skipped by its length
    if vid is None:
        raise ValueError("no video stream")
    if handler.upper() != b"MJPG" and comp.upper() != b"MJPG":
        raise ValueError("video codec %r / %r is not MJPG: only Motion-JPEG AVI can be decoded here" % (
            handler.decode("latin-1"), comp.decode("latin-1")))
    if movi is None:
        raise ValueError("no 'movi' list")
    ids = (b"%02ddc" % vid, b"%02ddb" % vid)
    frames = []
    if idx1 is not None:
        ent = [(buf[p:p + 4], _u32(buf, p + 8), _u32(buf, p + 12)) for p in range(idx1[0], idx1[1] - 15, 16)]
        ent = [e for e in ent if e[0] in ids]
        if ent:
            base = None
            for b in (movi[0], 0):                      # offsets count from the 'movi' tag, or (some writers) from the file's start
                o = b + ent[0][1]
                if o + 8 <= n and buf[o:o + 4] == ent[0][0]:
                    base = b
                    break
            if base is not None and all(base + o + 8 + s <= n for _, o, s in ent):
                frames = [(base + o + 8, s) for _, o, s in ent]
                info["indexed"] = True
    if not frames:                                      # no usable idx1: walk the movi list
        p, end = movi[0] + 4, movi[1]
        while p + 8 <= end:
            cc, size = buf[p:p + 4], _u32(buf, p + 4)
            if cc == b"LIST":                           # 'rec ' groups: step inside
                p += 12
                continue
            if cc in ids:
                if p + 8 + size > n:
                    break
                frames.append((p + 8, size))
            p += 8 + size + (size & 1)
    info["frames"] = frames
    info["fps"] = rate / scale if rate > 0 and scale > 0 else (1e6 / usec if usec > 0 else 30.0)
    return info


def _headers_end(buf, pos, n):
    """From a frame's SOI at pos: the offset behind its SOS header, or -1."""
    p = pos + 2
    while p + 4 <= n:
        if buf[p] != 0xFF:
            return -1
        m = buf[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            p += 2
            continue
        if m == 0xD9:
            return -1
        L = buf[p + 2] * 256 + buf[p + 3]
        if L < 2:
            return -1
        p += 2 + L
        if m == 0xDA:
            return p if p <= n else -1
    return -1


def index_mjpeg(buf):
    """Frames from each SOI to its EOI: header segments are stepped over by their length (a thumbnail in an APPn segment is not a
    frame); behind the SOS header the next FF D9 is the EOI, since entropy-coded data holds FF only before 00 or a restart marker."""
    n, frames, pos = len(buf), [], 0
    while True:
        pos = buf.find(b"\xff\xd8", pos)
        if pos < 0:
            break
        scan = _headers_end(buf, pos, n)
        if scan < 0:
            pos += 2
            continue
        eoi = buf.find(b"\xff\xd9", scan)
        end = n if eoi < 0 else eoi + 2
        frames.append((pos, end - pos))
        pos = end
    return frames


def jpeg_size(buf, offset, length):
    p, n = offset + 2, offset + length
    while p + 4 <= n and buf[p] == 0xFF:
        m = buf[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            p += 2
            continue
        L = buf[p + 2] * 256 + buf[p + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC) and p + 9 <= n:
            return buf[p + 7] * 256 + buf[p + 8], buf[p + 5] * 256 + buf[p + 6]
        if m == 0xDA or L < 2:
            break
        p += 2 + L
    return None


class AviWriter:
    """RIFF AVI 1.0 with one MJPG video stream, what index_avi reads: hdrl (avih, one strl: strh `vids` / `MJPG` + strf), a `movi` list
    of `00dc` chunks padded to even length, and idx1 (offsets relative to the `movi` tag).  add(data) appends one JPEG frame;
    close() writes idx1 and patches the frame count, the largest frame and the list sizes.  The file stays below 2 GB (AVI 1.0 without
    OpenDML): the add() that would cross it raises ValueError and writes nothing."""
    LIMIT = (1 << 31) - 1

    def __init__(self, path, fps, width, height):
        w, h, fps = int(width), int(height), float(fps)
        if w <= 0 or h <= 0 or not fps > 0:
            raise ValueError("AviWriter: bad size %dx%d or fps %r" % (w, h, fps))
        self.width, self.height, self.fps = w, h, fps
        self._rate, self._scale = int(round(fps * 1000)), 1000
        self._index, self._largest = [], 0
        self._f = open(path, "wb")
        self._f.write(self._head())
        self._movi = self._f.tell() - 4                 # offset of the 'movi' tag
        self._pos = self._f.tell()

    frames = property(lambda self: len(self._index))
    bytes_written = property(lambda self: self._pos)

    def _head(self, movi_bytes=4, riff_bytes=0):
        n, w, h = len(self._index), self.width, self.height
        avih = struct.pack("<14I", int(round(1e6 / self.fps)), 0, 0, 0x10, n, 0, 1, self._largest, w, h, 0, 0, 0, 0)
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4h", 0, 0, 0, 0, self._scale, self._rate, 0, n, self._largest, 0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        return (b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl +
                b"LIST" + struct.pack("<I", movi_bytes) + b"movi")

    def _closing_bytes(self, frames):
        return 8 + 16 * frames                          # the idx1 chunk

    def add(self, data):
        if self._f is None:
            raise ValueError("AviWriter: the file is closed")
        n = len(data)
        if self._pos + 8 + n + (n & 1) + self._closing_bytes(len(self._index) + 1) > self.LIMIT:
            raise ValueError("AviWriter: the file would pass 2 GB, which needs OpenDML (not written here); start another file")
        self._f.write(b"00dc" + struct.pack("<I", n))
        self._f.write(data)
        if n & 1:
            self._f.write(b"\0")
        self._index.append((self._pos - self._movi, n))
        self._largest = max(self._largest, n)
        self._pos += 8 + n + (n & 1)

    def close(self):
        if self._f is None:
            return
        f, self._f = self._f, None
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
            f.write(b"".join(b"00dc" + struct.pack("<III", 0x10, o, n) for o, n in self._index))
            end = self._pos + self._closing_bytes(len(self._index))
            f.seek(0)
            f.write(self._head(self._pos - self._movi, end - 8))
        finally:
            f.close()
        self._pos = end
