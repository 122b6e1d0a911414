"""Float64 reference of ONE op of the YOLO network, and the per-element error bound a correct half / float32 kernel stays inside.

Plain NumPy / torch-CPU code, no GPU.  tests/test_gpu_yolo_layers.py reads an op's operands and output back from the device
(YoloV8n.ops(), the av_yolo_op hook) and holds the output against `conv_want` / `pools_want` / `upsample_want` with `bound`;
tests/test_yolo_layer_ref_host.py checks this file itself: an emulation of a correct kernel stays inside the bound, two planted
omissions fall outside it, and the per-op reference chained over the whole network is oracle/yolo_ref.py's network.

The bound per output element of a convolution with half output (K = taps * cin):

    |got - want| <= u_h |want| (1 + 2^-8) + 1.1 (K + 2) 2^-24 (sum |w x| + |b| + |res|) + 2^-25

u_h = 2^-11 is the unit roundoff of IEEE half (the final rounding; 2^-8 leaves room for the device's float32 sigmoid).  Products of
two halves are exact in float32, so the second term is the standard worst case of a float32 sum of K + 2 terms in ANY order -- which
covers the MFMA's internal order -- carried through SiLU, whose slope is at most 1.1.  2^-25 is half the subnormal step of half.
With a float32 output (the head's logits, the float32 mode) the first term is 2^-23 |want|.  The constants are derived, not tuned
to what a kernel gives.
"""
import numpy as np

U_H = 2.0 ** -11
U_S = 2.0 ** -24
SUBNORMAL = 2.0 ** -14          # below this a half has fewer than 11 significant bits: the bound is all absolute there

# the five shapes of tests/test_gpu_yolo_layers.py: frame size, network input size, batch, anchors
CASES = {
    "A": dict(frame=(64, 1280), net=(32, 640), batch=1, anchors=420),       # maps of 16, 8, 4, 2 and 1 rows
    "B": dict(frame=(1280, 64), net=(640, 32), batch=2, anchors=420),       # one- and two-column maps
    "C": dict(frame=(90, 333), net=(192, 640), batch=3, anchors=2520),      # generic letterbox up by 1.92, 9 + 10 padding rows, 6-row P5
    "D": dict(frame=(64, 1280), net=(32, 640), batch=64, anchors=420),      # P2 npix 81 920, 16-row tiles over 8-row maps
    "E": dict(frame=(720, 1280), net=(384, 640), batch=1, anchors=5040),    # the shape the path-against-path tests stand on
}


def case_frames(name):
    """The case's BGR frames, uint8 [batch, h, w, 3]: noise (every halo pixel matters) with constant plateaus and one flat
    rectangle (edges that do not sit on a tile border), different per image."""
    c = CASES[name]
    h, w = c["frame"]
    rs = np.random.RandomState(1000 + ord(name))
    out = rs.randint(0, 256, (c["batch"], h, w, 3)).astype(np.uint8)
    for b in range(c["batch"]):
        for _ in range(4):                                   # plateaus
            y, x = rs.randint(0, h - 8), rs.randint(0, w - 8)
            out[b, y:y + rs.randint(4, max(5, h // 3)), x:x + rs.randint(4, max(5, w // 3))] = rs.randint(0, 256, 3)
        y, x = rs.randint(0, h // 2), rs.randint(0, w // 2)
        out[b, y:y + h // 3, x:x + w // 3] = (40, 180, 90)  # the flat rectangle
    return out


def silu(v):
    v = np.asarray(v, np.float64)
    return v / (1.0 + np.exp(-v))


def _conv2d(x, w, stride, pad):
    """x float64 [B, H, W, cin], w float64 [cout, k, k, cin] -> [B, Ho, Wo, cout] (zero padding `pad`)."""
    import torch
    import torch.nn.functional as F
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))), torch.from_numpy(np.ascontiguousarray(w.transpose(0, 3, 1, 2))),
                 None, stride, pad)
    return y.numpy().transpose(0, 2, 3, 1)


def conv_want(x, w, b, stride, act, res=None, pad=None):
    """One convolution in float64: x [B, H, W, cin], w [cout, k, k, cin], b [cout], optional residual [B, Ho, Wo, cout] (added after the
    activation).  -> (want, mag) with mag = sum |w x| + |b| + |res|, the magnitude the accumulation error scales with."""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    pad = w.shape[1] // 2 if pad is None else pad
    want = _conv2d(x, w, stride, pad) + b
    mag = _conv2d(np.abs(x), np.abs(w), stride, pad) + np.abs(b)
    if act:
        want = silu(want)
    if res is not None:
        res = np.asarray(res, np.float64)
        want, mag = want + res, mag + np.abs(res)
    return want, mag


def bound(want, mag, K, out_f32=False):
    """The per-element bound of the module docstring."""
    first = 2.0 ** -23 * np.abs(want) if out_f32 else U_H * np.abs(want) * (1 + 2.0 ** -8)
    return first + 1.1 * (K + 2) * U_S * mag + 2.0 ** -25


def accumulation_ratio(got, want, mag, out_f32=False):
    """Information only: the largest (err - u |want|) / (2^-24 sum |w x|) -- how much of the worst-case accumulation term was used."""
    err = np.abs(np.asarray(got, np.float64) - want) - (2.0 ** -24 if out_f32 else U_H) * np.abs(want)
    return float((err / (U_S * np.maximum(mag, 1e-300))).max())


def maxpool5(x):
    """5x5 stride-1 maximum with -inf padding (F.max_pool2d(x, 5, 1, 2)), exact.  x [B, H, W, C]."""
    B, H, W, C = x.shape
    p = np.full((B, H + 4, W + 4, C), -np.inf, x.dtype)
    p[:, 2:-2, 2:-2] = x
    out = p[:, 0:H, 0:W].copy()
    for dy in range(5):
        for dx in range(5):
            np.maximum(out, p[:, dy:dy + H, dx:dx + W], out=out)
    return out


def pools_want(x):
    """SPPF's three chained pools: [B, H, W, 3 C]."""
    a = maxpool5(x)
    b = maxpool5(a)
    return np.concatenate([a, b, maxpool5(b)], axis=3)


def upsample_want(x):
    return x.repeat(2, axis=1).repeat(2, axis=2)


def nonvacuous(want):
    """(fraction of elements with |want| < 2^-14, fraction above a tenth of the map's maximum): the first must stay below a half, the
    second reach 1 %, or a comparison with `bound` says little about the op."""
    a = np.abs(want)
    return float((a < SUBNORMAL).mean()), float((a > 0.1 * a.max()).mean())


# ---- the network as a list of ops (the order and slices of the library's build_graph), for a chain on the host ----------------

def network_ops(f32=False):
    """-> (ops, bufs): ops = dicts {kind, in, out, k, s, act, res} with slices (buffer name, first channel, channels), in execution
    order; bufs = {name: (downscale of the network input, channels)}.  f32: SPPF's pools as three ops (the float32 mode's form)."""
    ops = []
    bufs = {"x0": (1, 3), "b0": (2, 16), "b1": (4, 32), "b2": (4, 32), "b3": (8, 64), "b5": (16, 128), "b7": (32, 256), "b8": (32, 256),
            "cat14": (8, 192), "cat11": (16, 384), "cat20": (32, 384), "cat17": (16, 192), "spp": (32, 512), "p3": (8, 64), "p4": (16, 128),
            "p5": (32, 256)}

    def conv(i, o, k, s, act=True, res=None):
        ops.append(dict(kind="conv", k=k, s=s, act=act, res=res, **{"in": i, "out": o}))

    def c2f(name, i, o, n, shortcut):
        c, div = o[2] // 2, bufs[i[0]][0]
        cat = name + ".cat"
        bufs[cat] = (div, (2 + n) * c)
        conv(i, (cat, 0, 2 * c), 1, 1)
        for j in range(n):
            tmp = "%s.tmp%d" % (name, j)
            bufs[tmp] = (div, c)
            src, dst = (cat, (1 + j) * c, c), (cat, (2 + j) * c, c)
            conv(src, (tmp, 0, c), 3, 1)
            conv((tmp, 0, c), dst, 3, 1, res=src if shortcut else None)
        conv((cat, 0, (2 + n) * c), o, 1, 1)

    conv(("x0", 0, 3), ("b0", 0, 16), 3, 2)
    conv(("b0", 0, 16), ("b1", 0, 32), 3, 2)
    c2f("l2", ("b1", 0, 32), ("b2", 0, 32), 1, True)
    conv(("b2", 0, 32), ("b3", 0, 64), 3, 2)
    c2f("l4", ("b3", 0, 64), ("cat14", 128, 64), 2, True)
    conv(("cat14", 128, 64), ("b5", 0, 128), 3, 2)
    c2f("l6", ("b5", 0, 128), ("cat11", 256, 128), 2, True)
    conv(("cat11", 256, 128), ("b7", 0, 256), 3, 2)
    c2f("l8", ("b7", 0, 256), ("b8", 0, 256), 1, True)
    conv(("b8", 0, 256), ("spp", 0, 128), 1, 1)
    if f32:
        for i in range(3):
            ops.append({"kind": "maxpool", "in": ("spp", 128 * i, 128), "out": ("spp", 128 * (i + 1), 128)})
    else:
        ops.append({"kind": "pools", "in": ("spp", 0, 128), "out": ("spp", 128, 384)})
    conv(("spp", 0, 512), ("cat20", 128, 256), 1, 1)
    ops.append({"kind": "upsample", "in": ("cat20", 128, 256), "out": ("cat11", 0, 256)})
    c2f("l12", ("cat11", 0, 384), ("cat17", 64, 128), 1, False)
    ops.append({"kind": "upsample", "in": ("cat17", 64, 128), "out": ("cat14", 0, 128)})
    c2f("l15", ("cat14", 0, 192), ("p3", 0, 64), 1, False)
    conv(("p3", 0, 64), ("cat17", 0, 64), 3, 2)
    c2f("l18", ("cat17", 0, 192), ("p4", 0, 128), 1, False)
    conv(("p4", 0, 128), ("cat20", 0, 128), 3, 2)
    c2f("l21", ("cat20", 0, 384), ("p5", 0, 256), 1, False)
    for lvl, (p, ch) in enumerate((("p3", 64), ("p4", 128), ("p5", 256))):
        div = bufs[p][0]
        for br, c in (("box", 64), ("cls", 80)):
            a, b, o = "h%d.%s.a" % (lvl, br), "h%d.%s.b" % (lvl, br), "h%d.%s" % (lvl, br)
            bufs[a], bufs[b], bufs[o] = (div, c), (div, c), (div, c)
            conv((p, 0, ch), (a, 0, c), 3, 1)
            conv((a, 0, c), (b, 0, c), 3, 1)
            conv((b, 0, c), (o, 0, c), 1, 1, act=False)
    return ops, bufs


# maps of oracle/yolo_ref.py's features(): name -> slice
NAMED = {"l1": ("b1", 0, 32), "l2": ("b2", 0, 32), "l4": ("cat14", 128, 64), "l6": ("cat11", 256, 128), "l8": ("b8", 0, 256),
         "l9": ("cat20", 128, 256), "l12": ("cat17", 64, 128), "p3": ("p3", 0, 64), "p4": ("p4", 0, 128), "p5": ("p5", 0, 256)}


def fold(params, dtype=np.float64):
    """Per convolution of conv_specs(): (w [cout, k, k, cin], bias [cout]) with BatchNorm (eps 1e-3) folded, the arithmetic of the
    library's fold_bn carried out in `dtype`: scale = g / sqrt(var + eps), w' = w scale, bias = beta - mean scale."""
    from oracle import yolo_ref as R
    out, pos = [], 0
    for cin, cout, k, _, bn in R.conv_specs():
        nw = cout * cin * k * k
        w = params[pos:pos + nw].reshape(cout, cin, k, k).astype(dtype)
        pos += nw
        if bn:
            g, be, mu, var = (params[pos + i * cout:pos + (i + 1) * cout].astype(dtype) for i in range(4))
            pos += 4 * cout
            scale = g / np.sqrt(var + dtype(1e-3))
            w, bias = w * scale[:, None, None, None], be - mu * scale
        else:
            bias = params[pos:pos + cout].astype(dtype)
            pos += cout
        out.append((np.ascontiguousarray(w.transpose(0, 2, 3, 1)), bias))
    assert pos == params.size
    return out


def run_chain(params, x, half=False, on_op=None):
    """The per-op float64 reference chained over the whole network.  x: the network input, float [B, H, W, 3] (RGB in [0, 1]).
    half: operands as the device holds them -- input, folded weights and every map rounded to IEEE half (logits stay float64).
    on_op(k, op, want, mag), if given, sees every op's result.  -> {buffer name: float64 [B, H / div, W / div, C]}."""
    ops, shapes = network_ops()
    rnd = (lambda a: a.astype(np.float16).astype(np.float64)) if half else (lambda a: a)
    B, H, W, _ = x.shape
    bufs = {n: np.zeros((B, H // d, W // d, c)) for n, (d, c) in shapes.items()}
    bufs["x0"][:] = rnd(np.asarray(x, np.float64))
    cut = lambda s: bufs[s[0]][..., s[1]:s[1] + s[2]]
    weights = iter(fold(np.asarray(params, np.float32)))
    for k, op in enumerate(ops):
        xin = cut(op["in"])
        if op["kind"] == "conv":
            w, b = next(weights)
            want, mag = conv_want(xin, rnd(w), b.astype(np.float32), op["s"], op["act"], None if op["res"] is None else cut(op["res"]))
            if op["act"]:
                want = rnd(want)
        else:
            want, mag = (pools_want(xin) if op["kind"] == "pools" else upsample_want(xin)), None
        if on_op:
            on_op(k, op, want, mag)
        cut(op["out"])[:] = want
    return bufs
