"""VideoDataLoader -- drop-in surface of data/loaders/video_loader.py for uncompressed video and Motion-JPEG.

The reference opens any container OpenCV can decode (cv2.VideoCapture, video_loader.py:43-57) and seeks with
CAP_PROP_POS_FRAMES per frame (:120).  Neither OpenCV nor any other decoder exists in this image, so this loader reads the
formats this library can decode itself and does the pixel work on the device:
  * `.y4m`  YUV4MPEG2, 4:2:0 planar (what `ffmpeg -pix_fmt yuv420p out.y4m` writes): frames are memory-mapped, a seek is
            an offset, I420 -> BGR (av_i420_to_bgr) and the resize to target_size (av_resize_into) run on the GPU;
  * `.npy`  uint8 array [frames, height, width, 3] (BGR), memory-mapped; resize on the GPU;
  * `.avi`  with an MJPG video stream, and `.mjpeg` / `.mjpg`, a raw concatenation of JPEG frames (`ffmpeg -c:v mjpeg`, dash cams,
            USB cameras): the file is memory-mapped and indexed once (video_index.py: idx1 or a walk of `movi`; SOI .. EOI), a seek is
            an index lookup; a batch's compressed bytes go up in one copy and av_jpeg_decode (baseline JPEG: Huffman decode, inverse
            DCT, chroma upsampling, colour conversion) leaves BGR frames in HBM.  The pixels are libjpeg's (islow IDCT, fancy
            upsampling).  A frame that does not decode cleanly reads as None, like a failed cap.read(); `last_status` tells why.
Inter-frame codecs (mp4 / mov / mkv, non-MJPG avi) raise ValueError naming the missing decoder.  Same properties and methods
as the reference class, plus read_frames_device() / read_frames_into(), which leave a batch of frames in HBM for the batched
pipeline, and VideoFeed, which reads frame k of S files in one decode call (what PerceptionLoop / CameraLoop step on).

The way out, where the reference hands its annotated frames to cv2.VideoWriter (demo.py:84-90, :170):
  * MJPEGWriter  Motion-JPEG, `.avi` (video_index.AviWriter) or a raw `.mjpeg` / `.mjpg` stream: a batch is encoded on the device in one
                 av_jpeg_encode call (baseline JPEG, byte for byte libjpeg's / Pillow's frames), and only the compressed bytes come down,
                 about 0.1 byte per pixel.  Any player and browser opens the file, and so does the loader above;
  * Y4MWriter    uncompressed 4:2:0 `.y4m` (av_bgr_to_i420, 1.5 bytes per pixel), which the loader above (or ffmpeg) reads.
Grayscale, progressive and optimised-Huffman JPEG are not written.
"""
import ctypes as C
import mmap
from pathlib import Path
from typing import Generator, Optional, Tuple

import numpy as np
import torch

from . import _native as nat
from . import video_index
from ._dev import Dev


class JpegBatchDecoder:
    """Staging for av_jpeg_decode at one frame size: a pinned host buffer [descriptors | frame bytes | segment table] with its device
    copy, and the workspace.  decode() copies the frames' bytes into the pinned buffer, parses them there (av_jpeg_parse), uploads the
    used part once and enqueues the decode; nothing waits for the device except for the previous call's upload, before the pinned
    buffer is written again (and for the previous decode, where a device buffer has to grow or the caller changes the stream: device
    buffers are allocated on the stream that uses them).
    status: int32 [n] on the device, of the last decode; host_rc: av_jpeg_parse's code per frame of the last decode; last_call: the
    arguments of the last av_jpeg_decode (n_frames, device buffer address, offset of the segment table in it, n_segs_total, max_segs,
    offset of the bytes, n_bytes), with which tools/mjpegtime.py replays the kernels on the buffers already uploaded."""

    def __init__(self, dev, h, w):
        self.dev, self.h, self.w = dev, int(h), int(w)
        self.seg_cap = ((self.w + 7) // 8) * ((self.h + 7) // 8)
        self._pin = self._buf = self._ws = self._uploaded = self._decoded = self._stream_id = None
        self.status, self.host_rc, self.last_call = None, [], None

    def decode(self, frames, dst, stream=None):
        """frames: n bytes-like objects, one JPEG frame each; dst: uint8 device tensor [n, h, w, 3], contiguous."""
        n, h, w, L = len(frames), self.h, self.w, self.dev.lib
        if (not torch.is_tensor(dst) or not dst.is_cuda or dst.dtype != torch.uint8 or tuple(dst.shape) != (n, h, w, 3)
                or not dst.is_contiguous()):
            raise ValueError("JpegBatchDecoder.decode: dst must be a contiguous uint8 device tensor [%d, %d, %d, 3]" % (n, h, w))
        lens = [len(f) for f in frames]
        desc_bytes = (n * nat.JPEG_DESC_BYTES + 15) & ~15
        data_bytes = sum((x + 3) & ~3 for x in lens) + 8
        need = desc_bytes + data_bytes + n * self.seg_cap * 8
        if self._uploaded is not None:
            self._uploaded.synchronize()                                   # the previous upload still reads the pinned buffer
        if self._pin is None or self._pin.numel() < need:
            self._pin = torch.empty(need + need // 4, dtype=torch.uint8, pin_memory=True)
        host, base = self._pin.numpy(), self._pin.data_ptr()
        off, seg_off, total, max_segs, n_seg = desc_bytes, desc_bytes + data_bytes, 0, 1, C.c_int()
        host[off + data_bytes - 12:off + data_bytes] = 0                   # the padding behind the last frame
        self.host_rc = []
        for k, f in enumerate(frames):
            host[off:off + lens[k]] = np.frombuffer(f, np.uint8)
            dp = base + k * nat.JPEG_DESC_BYTES
            rc = L.av_jpeg_parse(base + off, lens[k], h, w, dp, base + seg_off + total * 8, self.seg_cap, C.byref(n_seg)) if lens[k] else \
                nat.EJPEG_TRUNCATED
            self.host_rc.append(int(rc))
            if rc != 0:
                C.memset(dp, 0, nat.JPEG_DESC_BYTES)                       # no frame of this size: the kernels leave it mid-gray
            else:
                d = nat.JpegDesc.from_address(dp)
                d.seg_base, d.byte_base = total, off - desc_bytes
                total += n_seg.value
                max_segs = max(max_segs, n_seg.value)
            off += (lens[k] + 3) & ~3
        used = seg_off + max(total, 1) * 8
        ws = int(L.av_jpeg_workspace_bytes(n, h, w))
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(self.dev.device):
            cur = torch.cuda.current_stream(self.dev.device)
            grow = self._buf is None or self._buf.numel() < self._pin.numel() or self._ws is None or self._ws.numel() < ws
            if self._decoded is not None and (grow or self._stream_id != cur.cuda_stream):
                self._decoded.synchronize()                                # before a buffer the previous decode uses goes back to the allocator
            self._stream_id = cur.cuda_stream
            if self._buf is None or self._buf.numel() < self._pin.numel():
                self._buf = torch.empty(self._pin.numel(), dtype=torch.uint8, device=self.dev.device)
            if self._ws is None or self._ws.numel() < ws:
                self._ws = torch.empty(ws, dtype=torch.uint8, device=self.dev.device)
            self._buf[:used].copy_(self._pin[:used], non_blocking=True)
            self._uploaded = torch.cuda.Event()
            self._uploaded.record(cur)
            self.status = torch.empty(n, dtype=torch.int32, device=self.dev.device)
            b = self._buf.data_ptr()
            nat.check(L.av_jpeg_decode(self.dev.ctx.handle, nat.stream_handle(cur), n, h, w, b, b + seg_off, max(total, 1), max_segs,
                                       b + desc_bytes, data_bytes, nat.ptr(self._ws), nat.ptr(dst), nat.ptr(self.status)))
            self._decoded = torch.cuda.Event()
            self._decoded.record(cur)
        self.last_call = (n, b, seg_off, max(total, 1), max_segs, desc_bytes, data_bytes)

    def last_status(self):
        """int32 [n]: 0 for a clean frame, AV_JPEG_E* bits from the device, or av_jpeg_parse's negative code.  Waits for the decode."""
        if self.status is None:
            return np.zeros(0, np.int32)
        self._decoded.synchronize()
        st = self.status.cpu().numpy().copy()
        for k, rc in enumerate(self.host_rc):
            if rc != 0:
                st[k] = rc
        return st


class VideoDataLoader:
    def __init__(self, video_path: str, target_size: Optional[Tuple[int, int]] = None, device: int = 0):
        self.video_path = Path(video_path)
        self.target_size = target_size
        self.cap = None
        self.frame_count = 0
        self._status = self._map = self._file = None
        if not self.video_path.exists():
            raise FileNotFoundError("Video file not found: %s" % video_path)
        self._dev = Dev(device)
        self._open_video()

    def _open_video(self):
        suf = self.video_path.suffix.lower()
        if suf == ".npy":
            arr = np.load(str(self.video_path), mmap_mode="r")
            if arr.ndim != 4 or arr.shape[3] != 3 or arr.dtype != np.uint8:
                raise ValueError("Could not open video file: %s (expected uint8 [frames, h, w, 3])" % self.video_path)
            self._kind, self._arr, self._fps = "npy", arr, 30.0
            self._total_frames, self._height, self._width = int(arr.shape[0]), int(arr.shape[1]), int(arr.shape[2])
        elif suf == ".y4m":
            with open(self.video_path, "rb") as f:
                head = f.readline(256)
            if not head.startswith(b"YUV4MPEG2 "):
                raise ValueError("Could not open video file: %s (not a YUV4MPEG2 stream)" % self.video_path)
            w = h = 0
            fps, chroma = 30.0, "420"
            for tok in head.split()[1:]:
                t = tok.decode("ascii", "replace")
                if t[0] == "W":
                    w = int(t[1:])
                elif t[0] == "H":
                    h = int(t[1:])
                elif t[0] == "F" and ":" in t:
                    a, b = t[1:].split(":")
                    fps = float(a) / float(b) if float(b) else 30.0
                elif t[0] == "C":
                    chroma = t[1:]
            if not chroma.startswith("420") or w <= 0 or h <= 0 or w % 2 or h % 2:
                raise ValueError("Could not open video file: %s (only even-sized 4:2:0 Y4M is supported, got C%s %dx%d)" % (
                    self.video_path, chroma, w, h))
            self._kind, self._fps, self._width, self._height = "y4m", fps, w, h
            self._hdr, self._fsz = len(head), w * h * 3 // 2
            raw = np.memmap(str(self.video_path), np.uint8, mode="r")
            self._raw = raw
            self._total_frames = (len(raw) - self._hdr) // (6 + self._fsz)        # every frame: b"FRAME\n" + planes
            if self._total_frames <= 0 or bytes(raw[self._hdr:self._hdr + 6]) != b"FRAME\n":
                raise ValueError("Could not open video file: %s (no plain FRAME records)" % self.video_path)
        elif suf in (".avi", ".mjpeg", ".mjpg"):
            self._file = open(self.video_path, "rb")
            try:
                self._map = mmap.mmap(self._file.fileno(), 0, access=mmap.ACCESS_READ)
            except ValueError:
                raise ValueError("Could not open video file: %s (empty file)" % self.video_path) from None
            try:
                if suf == ".avi":
                    info = video_index.index_avi(self._map)
                    frames, w, h, fps = info["frames"], info["width"], info["height"], info["fps"]
                else:
                    frames, fps = video_index.index_mjpeg(self._map), 30.0
                    size = video_index.jpeg_size(self._map, *frames[0]) if frames else None
                    w, h = size if size else (0, 0)
            except ValueError as e:
                raise ValueError("Could not open video file: %s (%s)" % (self.video_path, e)) from None
            if not frames or w <= 0 or h <= 0:
                raise ValueError("Could not open video file: %s (no JPEG frames found)" % self.video_path)
            self._kind, self._index, self._fps, self._width, self._height = "mjpeg", frames, float(fps), int(w), int(h)
            self._total_frames = len(frames)
            self._jpeg = JpegBatchDecoder(self._dev, h, w)
        else:
            raise ValueError("Could not open video file: %s -- %s needs a bitstream decoder (OpenCV / FFmpeg / VCN), none is "
                             "available here; convert to .y4m (4:2:0), .npy or Motion-JPEG (.avi / .mjpeg)" % (self.video_path, suf or "this format"))
        self.cap = self
        self._duration = self._total_frames / self._fps if self._fps > 0 else 0

    # ---- properties (video_loader.py:59-87) ------------------------------------------------------------------------
    total_frames = property(lambda self: self._total_frames)
    fps = property(lambda self: self._fps)
    width = property(lambda self: self.target_size[0] if self.target_size else self._width)
    height = property(lambda self: self.target_size[1] if self.target_size else self._height)
    duration = property(lambda self: self._duration)
    dt = property(lambda self: 1.0 / self._fps if self._fps > 0 else 0.033)

    # ---- frames ---------------------------------------------------------------------------------------------------------
    def read_frames_device(self, first: int, count: int) -> Optional[torch.Tensor]:
        """Frames [first, first + count) as a uint8 tensor [count, height, width, 3] (BGR) in HBM: planes / pixels go up
        as they lie in the file, colour conversion and resize happen on the device."""
        if self.cap is None or first < 0 or count <= 0 or first + count > self._total_frames:
            return None
        d, h, w = self._dev, self._height, self._width
        self._status = None
        if self._kind == "npy":
            src = d.upload(np.array(self._arr[first:first + count]), np.uint8)            # copy out of the read-only map
        elif self._kind == "mjpeg":
            src = d.empty((count, h, w, 3), torch.uint8)
            self._jpeg.decode(self.frame_bytes(first, count), src)
            self._status = self._jpeg
        else:
            stride = 6 + self._fsz
            planes = np.stack([self._raw[self._hdr + k * stride + 6:self._hdr + (k + 1) * stride] for k in range(first, first + count)])
            yuv = d.upload(planes, np.uint8)
            src = d.empty((count, h, w, 3), torch.uint8)
            nat.check(d.lib.av_i420_to_bgr(d.ctx.handle, d.stream, count, h, w, nat.ptr(yuv), nat.ptr(src)))
        if self.target_size is None or tuple(self.target_size) == (w, h):
            return src
        tw, th = int(self.target_size[0]), int(self.target_size[1])
        out = d.empty((count, th, tw, 3), torch.uint8)
        for k in range(count):
            nat.check(d.lib.av_resize_into(d.ctx.handle, d.stream, nat.ptr(src[k]), h, w, nat.ptr(out[k]), th, tw, tw, 0))
        return out

    def frame_bytes(self, first: int, count: int) -> list:
        """The compressed bytes of the frames [first, first + count) of a Motion-JPEG file, as views into the mapped file."""
        with memoryview(self._map) as view:
            return [view[o:o + n] for o, n in self._index[first:first + count]]

    def read_frames_into(self, dst: torch.Tensor, first: int, count: int, stream=None) -> bool:
        """Frames [first, first + count) into the caller's uint8 device tensor [count, height, width, 3], enqueued on `stream` (a
        torch stream; default: the current one).  Motion-JPEG at its own size is decoded straight into dst; everything else goes
        through read_frames_device() on that stream and one device copy.  -> False (nothing enqueued) outside the file."""
        if self.cap is None or first < 0 or count <= 0 or first + count > self._total_frames:
            return False
        if tuple(dst.shape) != (count, self.height, self.width, 3):
            raise ValueError("read_frames_into: dst must be [%d, %d, %d, 3], got %s" % (count, self.height, self.width, tuple(dst.shape)))
        if self._kind == "mjpeg" and (self.target_size is None or tuple(self.target_size) == (self._width, self._height)):
            self._jpeg.decode(self.frame_bytes(first, count), dst, stream)
            self._status = self._jpeg
            return True
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(self._dev.device):
            dst.copy_(self.read_frames_device(first, count))
        return True

    @property
    def last_status(self) -> np.ndarray:
        """int32 per frame of the last batch read: 0 where the frame is good (always, for uncompressed files); for Motion-JPEG the
        AV_JPEG_E* bits of a damaged frame or av_jpeg_parse's negative code (include/avhot.h).  Waits for the decode."""
        return self._status.last_status() if self._status is not None else np.zeros(0, np.int32)

    def _one(self, idx):
        t = self.read_frames_device(idx, 1)
        if t is None:
            return None
        self.frame_count = idx + 1
        if self._kind == "mjpeg" and int(self.last_status[0]) != 0:
            return None                                                     # as when cap.read() fails
        return t[0].cpu().numpy()

    def read_frame(self) -> Optional[np.ndarray]:
        return self._one(self.frame_count)

    def read_frame_at(self, frame_idx: int) -> Optional[np.ndarray]:
        return self._one(frame_idx)

    def generate_frame_with_vehicles(self) -> Optional[np.ndarray]:
        return self.read_frame()

    def generate_video_stream(self, num_frames: Optional[int] = None) -> Generator[np.ndarray, None, None]:
        self.reset()
        n = num_frames if num_frames else self._total_frames
        for _ in range(n):
            frame = self.read_frame()
            if frame is None:
                break
            yield frame

    def generate_ego_motion(self, num_steps: Optional[int] = None) -> list:
        """Placeholder ego measurements (video_loader.py:166-205), drawn from the global NumPy stream like the reference."""
        if num_steps is None:
            num_steps = self._total_frames
        out, x, y, speed, dt = [], 0.0, 0.0, 10.0, self.dt
        for i in range(num_steps):
            heading = 0.05 * np.sin(i * dt * 0.5)
            vx, vy = speed * np.cos(heading), speed * np.sin(heading)
            x += vx * dt
            y += vy * dt
            out.append((x + np.random.normal(0, 0.1), y + np.random.normal(0, 0.1), vx + np.random.normal(0, 0.05),
                        vy + np.random.normal(0, 0.05)))
        return out

    def reset(self):
        self.frame_count = 0

    def release(self):
        self.cap = None
        if self._map is not None:                       # a Motion-JPEG file: the mapping and the file behind it
            self._map.close()
            self._file.close()
            self._map = self._file = None

    def __len__(self) -> int:
        return self._total_frames

    def __iter__(self):
        self.reset()
        return self

    def __next__(self) -> np.ndarray:
        frame = self.read_frame()
        if frame is None:
            raise StopIteration
        return frame

    def get_info(self) -> dict:
        return {"path": str(self.video_path), "total_frames": self._total_frames, "fps": self._fps, "width": self._width,
                "height": self._height, "duration": self._duration, "target_size": self.target_size}

    def __repr__(self) -> str:
        return "VideoDataLoader(path='%s', frames=%d, fps=%.1f, size=%dx%d)" % (self.video_path.name, self._total_frames, self._fps,
                                                                             self._width, self._height)


class VideoFeed:
    """Frame k of S video files of one frame size, read together: VideoFeed(paths_or_loaders, start=0).  read_into(dst, stream) puts
    frame k of every file into dst [S, height, width, 3] and advances k; the Motion-JPEG members are decoded in ONE av_jpeg_decode
    call (n_frames = S when all are), `.y4m` / `.npy` members go through their loaders.  len(feed) is the shortest file's frame
    count.  PerceptionLoop.step(frames=feed) / CameraLoop.step(frames=feed) decode straight into the loop's frame buffer."""

    def __init__(self, paths_or_loaders, start: int = 0, device: int = 0):
        self.loaders = [p if isinstance(p, VideoDataLoader) else VideoDataLoader(p, device=device) for p in paths_or_loaders]
        if not self.loaders:
            raise ValueError("VideoFeed: no files")
        sizes = sorted({(ld.width, ld.height) for ld in self.loaders})
        if len(sizes) != 1:
            raise ValueError("VideoFeed: the files have different frame sizes: %s" % ", ".join("%dx%d" % s for s in sizes))
        self.width, self.height = sizes[0]
        self.position = int(start)
        direct = [ld._kind == "mjpeg" and (ld.width, ld.height) == (ld._width, ld._height) for ld in self.loaders]
        self._jpeg_members = [i for i, on in enumerate(direct) if on]
        self._jpeg = JpegBatchDecoder(self.loaders[0]._dev, self.height, self.width) if self._jpeg_members else None

    def __len__(self) -> int:
        return min(len(ld) for ld in self.loaders)

    def reset(self, start: int = 0):
        self.position = int(start)

    def read_into(self, dst: torch.Tensor, stream=None):
        S, k = len(self.loaders), self.position
        if k < 0 or k >= len(self):
            raise IndexError("VideoFeed: frame %d of %d" % (k, len(self)))
        if tuple(dst.shape) != (S, self.height, self.width, 3):
            raise ValueError("VideoFeed.read_into: dst must be [%d, %d, %d, 3], got %s" % (S, self.height, self.width, tuple(dst.shape)))
        jm = self._jpeg_members
        if jm:
            frames = [self.loaders[i].frame_bytes(k, 1)[0] for i in jm]
            if len(jm) == S:
                self._jpeg.decode(frames, dst, stream)
            else:
                with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dst.device):
                    tmp = torch.empty((len(jm), self.height, self.width, 3), dtype=torch.uint8, device=dst.device)   # on the stream that uses it
                    self._jpeg.decode(frames, tmp, stream)
                    for j, i in enumerate(jm):
                        dst[i].copy_(tmp[j])
        for i, ld in enumerate(self.loaders):
            if i not in jm:
                ld.read_frames_into(dst[i:i + 1], k, 1, stream)
        self.position = k + 1

    @property
    def last_status(self) -> np.ndarray:
        """int32 [S] of the last read_into(): 0, or what VideoDataLoader.last_status reports for a Motion-JPEG frame."""
        st = np.zeros(len(self.loaders), np.int32)
        if self._jpeg is not None and self._jpeg.status is not None:
            st[self._jpeg_members] = self._jpeg.last_status()
        return st


class Y4MWriter:
    """Uncompressed YUV4MPEG2 4:2:0 video file.  Y4MWriter(path, fps, (width, height)); write(frame) takes one BGR frame on the host
    like cv2.VideoWriter.write, write_device(batch) a uint8 device tensor [n, height, width, 3] (one conversion launch, one
    download); release() closes the file.  4:2:0 needs even sizes (ValueError otherwise)."""

    def __init__(self, path: str, fps: float, size: Tuple[int, int], device: int = 0):
        w, h = int(size[0]), int(size[1])
        if w <= 0 or h <= 0 or w % 2 or h % 2:
            raise ValueError("Y4MWriter: 4:2:0 needs even sizes, got %dx%d" % (w, h))
        from fractions import Fraction
        fr = Fraction(float(fps)).limit_denominator(1001)
        if fr <= 0:
            raise ValueError("Y4MWriter: fps must be positive")
        self.path, self.fps, self.width, self.height = Path(path), float(fps), w, h
        self._dev = Dev(device)
        self._f = open(self.path, "wb")
        self._f.write(b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg\n" % (w, h, fr.numerator, fr.denominator))

    def write_device(self, batch: torch.Tensor):
        if self._f is None:
            raise ValueError("Y4MWriter: the file is closed")
        if (not torch.is_tensor(batch) or not batch.is_cuda or batch.dtype != torch.uint8 or batch.dim() != 4
                or tuple(batch.shape[1:]) != (self.height, self.width, 3)):
            raise ValueError("Y4MWriter.write_device: expected a uint8 device tensor [n, %d, %d, 3]" % (self.height, self.width))
        n = int(batch.shape[0])
        if n == 0:
            return
        d = self._dev
        batch = batch.contiguous()
        fsz = self.width * self.height * 3 // 2
        yuv = d.empty((n, fsz), torch.uint8)
        nat.check(d.lib.av_bgr_to_i420(d.ctx.handle, d.stream, n, self.height, self.width, nat.ptr(batch), nat.ptr(yuv)))
        host = yuv.cpu().numpy()
        for k in range(n):
            self._f.write(b"FRAME\n")
            self._f.write(host[k].tobytes())

    def write(self, frame: np.ndarray):
        frame = np.ascontiguousarray(frame, np.uint8)
        if frame.shape != (self.height, self.width, 3):
            raise ValueError("Y4MWriter.write: expected a %dx%dx3 uint8 frame, got shape %s" % (self.height, self.width, frame.shape))
        self.write_device(self._dev.upload(frame[None], np.uint8))

    def release(self):
        if self._f is not None:
            self._f.close()
            self._f = None


class MJPEGWriter:
    """Motion-JPEG video file, encoded on the device.  MJPEGWriter(path, fps, (width, height), quality=85, subsampling="420" | "422" |
    "444", restart_mcus=-1 (one restart interval per MCU row; 0: none; else MCUs per interval)); write(frame) takes one BGR frame on
    the host like cv2.VideoWriter.write, write_device(batch) a uint8 device tensor [n, height, width, 3]: one av_jpeg_encode call, a
    download of the lengths, then of the used bytes only.  `.avi` gives an AVI with an MJPG stream, `.mjpeg` / `.mjpg` the frames one
    behind the other.  release() (or leaving the `with` block) finishes the file.  Every frame is what libjpeg writes for the same
    pixels and parameters; odd sizes are fine."""

    def __init__(self, path: str, fps: float, size: Tuple[int, int], quality: int = 85, subsampling: str = "420", restart_mcus: int = -1,
                 device: int = 0):
        w, h = int(size[0]), int(size[1])
        self.path = Path(path)
        suf = self.path.suffix.lower()
        if suf not in (".avi", ".mjpeg", ".mjpg"):
            raise ValueError("MJPEGWriter: %s is neither .avi nor .mjpeg / .mjpg" % self.path.name)
        if subsampling not in nat.JPEG_SUBSAMPLING:
            raise ValueError("MJPEGWriter: subsampling must be one of '420', '422', '444', got %r" % (subsampling,))
        if not float(fps) > 0:
            raise ValueError("MJPEGWriter: fps must be positive")
        self.fps, self.width, self.height, self.quality, self.subsampling = float(fps), w, h, int(quality), subsampling
        self.restart_mcus, self._sub = int(restart_mcus), nat.JPEG_SUBSAMPLING[subsampling]
        head, qt = (C.c_uint8 * nat.JPEG_HEADER_MAX)(), (C.c_uint8 * 128)()
        n = nat.lib().av_jpeg_encode_header(h, w, self.quality, self._sub, self.restart_mcus, head, nat.JPEG_HEADER_MAX, qt)
        if n < 0:
            raise ValueError("MJPEGWriter: %s" % nat.lib().av_last_error_string().decode())
        self._dev = Dev(device)
        self._header_len = int(n)
        const = np.zeros(128 + nat.JPEG_HEADER_MAX, np.uint8)                  # quantisers, then the header: one upload
        const[:128], const[128:128 + n] = np.frombuffer(qt, np.uint8), np.frombuffer(head, np.uint8)[:n]
        self._const = self._dev.upload(const, np.uint8)
        self._ws = None
        self._cap = h * w                                                      # bytes per frame slot; grows when a frame needs more
        self._frames = self._bytes = 0
        self.last_call = None                                                  # (n, out_cap, retried) of the last write_device
        self._avi = video_index.AviWriter(str(self.path), self.fps, w, h) if suf == ".avi" else None
        self._f = None if self._avi else open(self.path, "wb")
        self._open = True

    frames_written = property(lambda self: self._frames)
    bytes_written = property(lambda self: self._avi.bytes_written if self._avi else self._bytes)

    def _encode(self, batch, n, cap):
        d, L = self._dev, self._dev.lib
        out = d.empty((n, cap), torch.uint8)
        info = d.empty((2, n), torch.int32)
        c = self._const.data_ptr()
        nat.check(L.av_jpeg_encode(d.ctx.handle, d.stream, n, self.height, self.width, nat.ptr(batch), c, self._sub, self.restart_mcus, c + 128,
                                   self._header_len, nat.ptr(self._ws), nat.ptr(out), cap, nat.ptr(info[0]), nat.ptr(info[1])))
        return out, info.cpu().numpy()

    def write_device(self, batch: torch.Tensor):
        if not self._open:
            raise ValueError("MJPEGWriter: the file is closed")
        if (not torch.is_tensor(batch) or not batch.is_cuda or batch.dtype != torch.uint8 or batch.dim() != 4
                or tuple(batch.shape[1:]) != (self.height, self.width, 3)):
            raise ValueError("MJPEGWriter.write_device: expected a uint8 device tensor [n, %d, %d, 3]" % (self.height, self.width))
        n = int(batch.shape[0])
        if n == 0:
            return
        d = self._dev
        batch = batch.contiguous()
        ws = int(d.lib.av_jpeg_encode_workspace_bytes(n, self.height, self.width, self._sub))
        if self._ws is None or self._ws.numel() < ws:
            self._ws = d.empty((ws,), torch.uint8)
        out, (lens, status) = self._encode(batch, n, self._cap)
        retried = bool((status & nat.JPEG_EFULL).any())
        if retried:                                                            # once more, sized by what the frames need
            self._cap = (int(lens.max()) + 4095) & ~4095
            out, (lens, status) = self._encode(batch, n, self._cap)
        if status.any():
            raise RuntimeError("MJPEGWriter: av_jpeg_encode status %s" % status.tolist())
        self.last_call = (n, self._cap, retried)
        used = int(lens.max())
        host = out[:, :used].cpu().numpy()                                     # only the bytes the longest frame uses
        for k in range(n):
            data = host[k, :int(lens[k])].tobytes()
            if self._avi:
                self._avi.add(data)
            else:
                self._f.write(data)
                self._bytes += len(data)
            self._frames += 1

    def write(self, frame: np.ndarray):
        if not self._open:
            raise ValueError("MJPEGWriter: the file is closed")
        if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.shape != (self.height, self.width, 3):
            raise ValueError("MJPEGWriter.write: expected a %dx%dx3 uint8 frame, got %s %s" % (
                self.height, self.width, getattr(frame, "dtype", type(frame).__name__), getattr(frame, "shape", "")))
        self.write_device(self._dev.upload(np.ascontiguousarray(frame)[None], np.uint8))

    def release(self):
        if self._open:
            self._open = False
            if self._avi:
                self._avi.close()
            else:
                self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
