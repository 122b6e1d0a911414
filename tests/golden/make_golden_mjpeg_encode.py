"""Writes tests/golden/mjpeg_encode.npz: frames and the bytes Pillow (libjpeg-turbo) encodes them to, the oracle of tests/jpeg_enc_ref.py
and of av_jpeg_encode.  Needs Pillow; the tests only read the .npz.

    python tests/golden/make_golden_mjpeg_encode.py

Per case `name`: rgb_<name> (uint8 [h, w, 3]), jpeg_<name> (Pillow's bytes), params_<name> (int32: quality, subsampling 0 / 1 / 2 for
4:4:4 / 4:2:2 / 4:2:0, restart_mcus as av_jpeg_encode_header takes it), and for the cases of `video` dec_<name>, Pillow's decode of its
own bytes.  `names` lists the cases, `video` four frames of one size and one parameter set, `full` three more (the out_cap cases),
`reached` what the set exercises (asserted below)."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import jpeg_enc_ref as er  # noqa: E402
from tests import jpeg_ref as jr  # noqa: E402

SUBS = ("444", "422", "420")


def content(kind, h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "mix":            # gradient + noise
        base = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // max(w + h - 2, 1)], 2)
        return np.clip(base + rng.randint(-24, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind in ("checker3", "checker8"):
        p = 3 if kind == "checker3" else 8
        return np.repeat((((xx // p + yy // p) & 1) * 255)[:, :, None], 3, 2).astype(np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([200, 40, 90], np.uint8), (h, w, 3)).copy()
    raise ValueError(kind)


def pillow(rgb, quality, sub, restart):
    kw = {}
    if restart == "rows":
        kw["restart_marker_rows"] = 1
    elif restart:
        kw["restart_marker_blocks"] = int(restart)
    b = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(b, "JPEG", quality=quality, subsampling=SUBS.index(sub), **kw)
    return b.getvalue()


def main():
    rng = np.random.RandomState(20241019)
    # name, w, h, content, subsampling, quality, restart ("rows", a number of MCUs, or None)
    cases = [("c16", 16, 16, "mix", "420", 85, "rows")]
    for (w, h) in ((17, 9), (37, 29)):
        for sub, q, rst in (("444", 95, None), ("422", 50, "rows"), ("420", 85, 1)):
            cases.append(("r%dx%d_%s" % (w, h, sub), w, h, "mix", sub, q, rst))
    cases += [
        ("d48x34", 48, 34, "mix", "420", 85, "rows"), ("d64x40", 64, 40, "noise", "420", 50, None),
        ("big_b1", 136, 72, "noise", "444", 100, 1),
        ("big_b3", 136, 72, "flat", "422", 95, 3), ("big_none", 136, 72, "checker8", "420", 5, None),
        ("t3x100", 3, 100, "mix", "420", 85, "rows"), ("t100x3", 100, 3, "noise", "422", 1, "rows"),
        ("chk3_q1", 40, 24, "checker3", "420", 1, None), ("chk3_q100", 40, 24, "checker3", "444", 100, "rows"),
        ("chk8_q100", 40, 24, "checker8", "422", 100, 3), ("noise_q5", 40, 24, "noise", "444", 5, "rows"),
        ("v0", 136, 72, "mix", "420", 85, "rows"), ("v1", 136, 72, "checker3", "420", 85, "rows"),
        ("v2", 136, 72, "flat", "420", 85, "rows"), ("v3", 136, 72, "checker8", "420", 85, "rows"),
        ("f0", 40, 24, "mix", "444", 100, 1), ("f1", 40, 24, "noise", "444", 100, 1), ("f2", 40, 24, "checker3", "444", 100, 1),
    ]
    video, full = ["v0", "v1", "v2", "v3"], ["f0", "f1", "f2"]
    out, stats, longer, n_intervals = {}, {}, [], {}
    for name, w, h, kind, sub, q, rst in cases:
        rgb = content(kind, h, w, rng)
        j = pillow(rgb, q, sub, rst)
        restart_mcus = -1 if rst == "rows" else int(rst or 0)
        bgr = np.ascontiguousarray(rgb[:, :, ::-1])
        mine = er.encode(bgr, q, sub, restart_mcus, stats)
        assert mine == j, "%s: the restatement differs from Pillow (%d vs %d bytes)" % (name, len(mine), len(j))
        coef, d = er.coefficients(bgr, q, sub)
        assert np.array_equal(coef, jr.decode_coefficients(j, h, w)[0]), name
        out["rgb_" + name], out["jpeg_" + name] = rgb, np.frombuffer(j, np.uint8)
        out["params_" + name] = np.array([q, SUBS.index(sub), restart_mcus], np.int32)
        if name in video:
            out["dec_" + name] = np.asarray(Image.open(io.BytesIO(j)).convert("RGB"))
        if len(j) > h * w:
            longer.append(name)
        n_intervals[name] = jr.parse(j, h, w)["n_segments"]
    # what the set has to reach
    assert stats["zrl"] > 0 and stats["no_eob"] > 0 and stats["ff"] > 0, stats
    assert {1, 2, 3, 4, 5, 6, 7} <= stats["pad_bits"], stats["pad_bits"]
    assert stats["dc_cat"] == 11 and stats["ac_cat"] == 10, (stats["dc_cat"], stats["ac_cat"])
    assert "f1" in longer and "big_b1" in longer, longer
    assert n_intervals["big_b1"] == 153 and n_intervals["big_none"] == 1 and n_intervals["v0"] == 5
    out["names"], out["video"], out["full"] = np.array([c[0] for c in cases]), np.array(video), np.array(full)
    out["reached"] = np.array([stats["dc_cat"], stats["ac_cat"], stats["zrl"], stats["no_eob"], stats["ff"]], np.int32)
    path = os.path.join(HERE, "mjpeg_encode.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases; reached", stats, "; longer than h*w:", longer)
    assert os.path.getsize(path) <= 256 * 1024


if __name__ == "__main__":
    main()
