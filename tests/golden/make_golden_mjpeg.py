"""Writes tests/golden/mjpeg.npz: baseline-JPEG frames encoded by Pillow (libjpeg-turbo) and Pillow's own decode of each, the oracle
of tests/jpeg_ref.py and of av_jpeg_decode.  Needs Pillow; the tests only read the .npz.

    python tests/golden/make_golden_mjpeg.py

Per case `name`: jpeg_<name> (uint8 bytes), rgb_<name> (uint8 [h, w, 3], Pillow's decode; gray replicated).  `names` lists the cases,
`video` the five frames of one 136 x 72 "video" in order."""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SUB = {"444": 0, "422": 1, "420": 2}


def content(kind, h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "mix":            # gradient + noise
        base = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)], 2)
        return np.clip(base + rng.randint(-24, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "checker":
        return np.repeat((((xx // 3 + yy // 3) & 1) * 255)[:, :, None], 3, 2).astype(np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([200, 40, 90], np.uint8), (h, w, 3)).copy()
    raise ValueError(kind)


def encode(img, sub, **kw):
    b = io.BytesIO()
    if sub == "gray":
        Image.fromarray(img[:, :, 1], "L").save(b, "JPEG", **kw)
    else:
        Image.fromarray(img, "RGB").save(b, "JPEG", subsampling=SUB[sub], **kw)
    return b.getvalue()


def strip_dht(j):
    """The frame without its DHT segments (what AVI MJPEG writers emit)."""
    out, pos = bytearray(j[:2]), 2
    while True:
        m, L = j[pos + 1], j[pos + 2] * 256 + j[pos + 3]
        if m != 0xC4:
            out += j[pos:pos + 2 + L]
        pos += 2 + L
        if m == 0xDA:
            return bytes(out) + j[pos:]


def main():
    rng = np.random.RandomState(20240607)
    cases = [("g8", 8, 8, "mix", "gray", dict(quality=90)), ("c16", 16, 16, "mix", "420", dict(quality=90))]
    for (w, h) in ((17, 9), (37, 29)):
        for sub in ("444", "422", "420", "gray"):
            cases.append(("r%dx%d_%s" % (w, h, sub), h, w, "mix", sub, dict(quality=50 if sub in ("422", "gray") else 90)))
    cases += [
        ("rst_rows", 34, 48, "mix", "420", dict(quality=85, restart_marker_rows=1)),
        ("rst_blocks", 72, 136, "noise", "444", dict(quality=100, restart_marker_blocks=1)),
        ("one_lane", 72, 136, "mix", "420", dict(quality=85)),
        ("noise_q1", 24, 40, "noise", "444", dict(quality=1)), ("noise_q5", 24, 40, "noise", "420", dict(quality=5)),
        ("checker_q1", 24, 40, "checker", "420", dict(quality=1)), ("checker_q5", 24, 40, "checker", "444", dict(quality=5)),
        ("optimize", 24, 40, "mix", "420", dict(quality=75, optimize=True)),
        ("no_dht", 24, 40, "mix", "420", dict(quality=75)),
        ("v0", 72, 136, "mix", "444", dict(quality=85, restart_marker_rows=1)), ("v1", 72, 136, "checker", "420", dict(quality=50)),
        ("v2", 72, 136, "flat", "422", dict(quality=90, restart_marker_blocks=3)), ("v3", 72, 136, "mix", "gray", dict(quality=30)),
        ("v4", 72, 136, "noise", "420", dict(quality=60, restart_marker_rows=2, optimize=True)),
    ]
    out = {}
    for name, h, w, kind, sub, kw in cases:
        j = encode(content(kind, h, w, rng), sub, **kw)
        if name == "no_dht":
            j = strip_dht(j)
            assert b"\xff\xc4" not in j[:j.index(b"\xff\xda")]
        out["jpeg_" + name] = np.frombuffer(j, np.uint8)
        out["rgb_" + name] = np.asarray(Image.open(io.BytesIO(j)).convert("RGB"))
        assert out["rgb_" + name].shape == (h, w, 3)
    out["names"] = np.array([c[0] for c in cases])
    out["video"] = np.array(["v0", "v1", "v2", "v3", "v4"])
    path = os.path.join(HERE, "mjpeg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")
    assert os.path.getsize(path) <= 256 * 1024


if __name__ == "__main__":
    main()
