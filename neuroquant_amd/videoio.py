"""Raw 8-bit YUV 4:2:0 video files on the host: YUV4MPEG2 (.y4m) and headerless planar I420 (.yuv).  numpy only, no GPU.

A frame is H * W * 3 / 2 bytes: the Y plane, then U, then V (what ops.frames_to_yuv420 writes and ops.yuv420_to_rgb_u8
reads).  Everything a file claims is checked here against the bytes it holds, so no byte count that the file does not back
ever reaches a kernel."""
import os
import re

import numpy as np

Y4M_MAGIC = b"YUV4MPEG2"
Y4M_CHROMA_420 = ("C420", "C420jpeg", "C420mpeg2", "C420paldv")
VIDEO_SUFFIXES = (".y4m", ".yuv")


def is_video_file(path):
    """True for a path that names a .y4m / .yuv file (by suffix); anything else is a directory of images to the drivers."""
    return isinstance(path, str) and path.lower().endswith(VIDEO_SUFFIXES)


def frame_bytes(H, W):
    """H * W * 3 / 2; ValueError for non-positive or odd sizes."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0 or H % 2 or W % 2:
        raise ValueError(f"4:2:0 frames need positive even sizes, got {W}x{H}")
    return H * W * 3 // 2


def parse_fps(text):
    """'30', '30000:1001' or '30000/1001' -> (num, den); ValueError otherwise."""
    m = re.fullmatch(r"(\d+)(?:[:/](\d+))?", str(text))
    if not m or int(m.group(1)) <= 0 or (m.group(2) is not None and int(m.group(2)) <= 0):
        raise ValueError(f"frame rate must be NUM or NUM:DEN with positive integers, got {text!r}")
    return int(m.group(1)), int(m.group(2) or 1)


def parse_size(text):
    """'WxH' -> (W, H); ValueError otherwise."""
    m = re.fullmatch(r"(\d+)[xX](\d+)", str(text))
    if not m:
        raise ValueError(f"size must be WxH, got {text!r}")
    return int(m.group(1)), int(m.group(2))


class write_y4m:
    """Context manager that writes a YUV4MPEG2 file of 8-bit 4:2:0 frames:

        with write_y4m(path, H, W, fps=(30, 1), full_range=False) as f:
            f.write(frames_u8)          # (k, H * W * 3 / 2) uint8, any number of times

    The header is 'YUV4MPEG2 W.. H.. Fnum:den Ip A1:1 C420jpeg XCOLORRANGE=LIMITED|FULL', every frame is 'FRAME' and its
    bytes.  raw=True writes the bytes alone (a .yuv file)."""

    def __init__(self, path, H, W, fps=(30, 1), full_range=False, raw=False):
        self.path, self.H, self.W = path, int(H), int(W)
        self.frame_bytes = frame_bytes(H, W)
        self.fps = (int(fps[0]), int(fps[1]))
        if self.fps[0] <= 0 or self.fps[1] <= 0:
            raise ValueError(f"frame rate must be positive, got {fps}")
        self.full_range, self.raw, self.frames, self._f = bool(full_range), bool(raw), 0, None

    def header(self):
        return "YUV4MPEG2 W{} H{} F{}:{} Ip A1:1 C420jpeg XCOLORRANGE={}\n".format(
            self.W, self.H, self.fps[0], self.fps[1], "FULL" if self.full_range else "LIMITED").encode("ascii")

    def __enter__(self):
        self._f = open(self.path, "wb")
        if not self.raw:
            self._f.write(self.header())
        return self

    def __exit__(self, *exc):
        self._f.close()
        self._f = None
        return False

    def write(self, frames_u8):
        a = np.asarray(frames_u8)
        if a.ndim == 1:
            a = a[None]
        if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != self.frame_bytes:
            raise ValueError(f"write_y4m: {self.W}x{self.H} frames are (k, {self.frame_bytes}) uint8, got {a.dtype} {a.shape}")
        if self._f is None:
            raise ValueError("write_y4m: use it as a context manager")
        for fr in a:
            if not self.raw:
                self._f.write(b"FRAME\n")
            self._f.write(np.ascontiguousarray(fr).tobytes())
            self.frames += 1


def open_writer(path, H, W, fps=(30, 1), full_range=False):
    """write_y4m for a .y4m path, the same frames without any header for .yuv."""
    return write_y4m(path, H, W, fps=fps, full_range=full_range, raw=path.lower().endswith(".yuv"))


class YuvFile:
    """An 8-bit 4:2:0 clip: H, W, frames, fps ((num, den) or None), full_range (True / False, None when the file does not say)
    and read(start, count) -> (count, H * W * 3 / 2) uint8."""

    def __init__(self, path, H, W, offsets, fps, full_range):
        self.path, self.H, self.W = path, H, W
        self.frame_bytes = frame_bytes(H, W)
        self._offsets, self.frames, self.fps, self.full_range = offsets, len(offsets), fps, full_range

    def read(self, start=0, count=None):
        start = int(start)
        count = self.frames - start if count is None else int(count)
        if start < 0 or count < 0 or start + count > self.frames:
            raise ValueError(f"{self.path}: frames [{start}, {start + count}) are not inside [0, {self.frames})")
        out = np.empty((count, self.frame_bytes), dtype=np.uint8)
        with open(self.path, "rb") as f:
            for i in range(count):
                f.seek(self._offsets[start + i])
                got = f.readinto(memoryview(out[i]))
                if got != self.frame_bytes:      # the file changed after it was indexed
                    raise ValueError(f"{self.path}: frame {start + i} is cut short ({got} of {self.frame_bytes} bytes)")
        return out


def _open_y4m(path):
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.readline(4096)
        if not head.endswith(b"\n") or not head.startswith(Y4M_MAGIC + b" "):
            raise ValueError(f"{path}: not a YUV4MPEG2 file")
        W = H = None
        fps, full_range = None, None
        for tag in head[len(Y4M_MAGIC):].decode("ascii", "replace").split():
            key, val = tag[0], tag[1:]
            if key == "W" and val.isdigit():
                W = int(val)
            elif key == "H" and val.isdigit():
                H = int(val)
            elif key == "F":
                m = re.fullmatch(r"(\d+):(\d+)", val)
                if not m:
                    raise ValueError(f"{path}: bad frame rate tag {tag!r}")
                fps = (int(m.group(1)), int(m.group(2)))
            elif key == "I":
                if val not in ("p", "?"):
                    raise ValueError(f"{path}: interlaced streams are not supported (tag {tag!r})")
            elif key == "C":
                if tag not in Y4M_CHROMA_420:
                    raise ValueError(f"{path}: only 8-bit 4:2:0 is supported (tag {tag!r})")
            elif key == "X" and val.startswith("COLORRANGE="):
                rng = val[len("COLORRANGE="):].upper()
                if rng not in ("FULL", "LIMITED"):
                    raise ValueError(f"{path}: unknown colour range (tag {tag!r})")
                full_range = rng == "FULL"
        if W is None or H is None:
            raise ValueError(f"{path}: the header gives no W / H")
        fb = frame_bytes(H, W)
        offsets = []
        pos = f.tell()
        while pos < size:
            f.seek(pos)
            line = f.readline(256)
            if not line.endswith(b"\n") or not (line == b"FRAME\n" or line.startswith(b"FRAME ")):
                raise ValueError(f"{path}: no FRAME line at byte {pos} (frame {len(offsets)})")
            pos += len(line)
            if pos + fb > size:
                raise ValueError(f"{path}: frame {len(offsets)} is cut short ({size - pos} of {fb} bytes)")
            offsets.append(pos)
            pos += fb
    return YuvFile(path, H, W, offsets, fps, full_range)


def _open_raw(path, size):
    if size is None:
        m = re.search(r"_(\d+)x(\d+)[_.]", os.path.basename(path))
        if not m:
            raise ValueError(f"{path}: a raw .yuv file needs size=(W, H) or a _<W>x<H> in its name")
        size = (int(m.group(1)), int(m.group(2)))
    W, H = int(size[0]), int(size[1])
    fb = frame_bytes(H, W)
    total = os.path.getsize(path)
    if total % fb:
        raise ValueError(f"{path}: {total} bytes are not a whole number of {W}x{H} 4:2:0 frames ({fb} bytes each)")
    return YuvFile(path, H, W, [i * fb for i in range(total // fb)], None, None)


def open_yuv(path, size=None):
    """Open a .y4m or raw .yuv clip of 8-bit 4:2:0 frames -> YuvFile.

    .y4m: the header and every FRAME line are parsed.  C420, C420jpeg, C420mpeg2 and C420paldv are accepted (no C tag means
    C420jpeg); they differ only in where the chroma samples are sited, and the siting is IGNORED: every chroma sample is
    taken to sit at the centre of its 2 x 2 block.  XCOLORRANGE=FULL|LIMITED sets full_range.  ValueError naming the tag for
    an interlaced stream, any other chroma format or bit depth (C422, C444, C420p10, Cmono, ...), and for a frame the file
    does not hold in full.
    .yuv: the size comes from size=(W, H) or from a _<W>x<H> followed by '_' or '.' in the file name; ValueError if neither
    gives it or the file length is not a whole number of frames."""
    if path.lower().endswith(".y4m"):
        f = _open_y4m(path)
        if size is not None and (f.W, f.H) != (int(size[0]), int(size[1])):
            raise ValueError(f"{path}: the header says {f.W}x{f.H}, size says {size[0]}x{size[1]}")
        return f
    return _open_raw(path, size)


def centre_crop_offsets(H, W, h, w):
    """(top, left) of the centre crop the drivers take from images; ValueError if the clip is smaller than the crop."""
    if H < h or W < w:
        raise ValueError(f"the clip is {W}x{H}, smaller than the crop {w}x{h}")
    return int(round((H - h) / 2.0)), int(round((W - w) / 2.0))


def crop_yuv420(frames_u8, H, W, top, left, h, w):
    """(k, H * W * 3 / 2) uint8 -> (k, h * w * 3 / 2): rows [top, top + h) and columns [left, left + w) of the Y plane and the
    chroma planes at half those offsets.  ValueError unless top, left, h and w are even and the window lies in the frame."""
    if top % 2 or left % 2:
        raise ValueError(f"a 4:2:0 crop needs even top and left offsets, got top={top}, left={left}")
    fb, fbc = frame_bytes(H, W), frame_bytes(h, w)
    if top < 0 or left < 0 or top + h > H or left + w > W:
        raise ValueError(f"crop {w}x{h} at ({top}, {left}) does not lie in a {W}x{H} frame")
    a = np.asarray(frames_u8)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != fb:
        raise ValueError(f"{W}x{H} frames are (k, {fb}) uint8, got {a.dtype} {a.shape}")
    if (top, left, h, w) == (0, 0, H, W):
        return a
    k, HW, hw = a.shape[0], H * W, h * w
    out = np.empty((k, fbc), dtype=np.uint8)
    out[:, :hw] = a[:, :HW].reshape(k, H, W)[:, top:top + h, left:left + w].reshape(k, hw)
    for p in range(2):
        src = a[:, HW + p * (HW // 4):HW + (p + 1) * (HW // 4)].reshape(k, H // 2, W // 2)
        out[:, hw + p * (hw // 4):hw + (p + 1) * (hw // 4)] = \
            src[:, top // 2:top // 2 + h // 2, left // 2:left // 2 + w // 2].reshape(k, hw // 4)
    return out
