"""tests/yolo_layer_ref.py checked on the host: the bound holds for a correct kernel's arithmetic and not for two planted omissions,
the per-op reference chained over the network is oracle/yolo_ref.py's network, float32 folding gives the half weights float64 folding
gives, and every op of every case of tests/test_gpu_yolo_layers.py has outputs large enough for the bound to mean something."""
import numpy as np
import pytest

from tests import yolo_layer_ref as L

ROWS = 4000


def _emulate(K, rs, out_f32=False, keep=None, with_res=False):
    """ROWS dot products of length K the way a correct kernel does them: half operands (float32 in the float32 variant), products and
    a SEQUENTIAL sum in float32, float32 bias, SiLU (evaluated in float64), optional residual, one rounding to the output type.
    keep: boolean [K] of the inputs the kernel does not drop (a planted bug).  -> (got, want, mag) as float64 [ROWS]."""
    t = np.float32 if out_f32 else np.float16
    x = L.silu(rs.standard_normal((ROWS, K))).astype(t)                                  # activations: SiLU of unit normals
    w = (rs.standard_normal((ROWS, K)) * np.sqrt(2.0 / K)).astype(t)                     # He-normal weights
    b = rs.uniform(-0.1, 0.1, ROWS).astype(np.float32)
    res = L.silu(rs.standard_normal(ROWS)).astype(t) if with_res else None
    acc = np.zeros(ROWS, np.float32)
    for k in range(K):
        if keep is None or keep[k]:
            acc = (acc + x[:, k].astype(np.float32) * w[:, k].astype(np.float32)).astype(np.float32)
    got = L.silu((acc + b).astype(np.float32))
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    want, mag = L.silu((x64 * w64).sum(1) + b), np.abs(x64 * w64).sum(1) + np.abs(b)
    if with_res:
        got, want, mag = got + res.astype(np.float32), want + res, mag + np.abs(res.astype(np.float64))
    return got.astype(t).astype(np.float64), want, mag


@pytest.mark.parametrize("K", [27, 288, 720, 2304])
def test_a_correct_kernels_arithmetic_stays_inside_the_bound(K):
    rs = np.random.RandomState(K)
    for res in (False, True):
        got, want, mag = _emulate(K, rs, with_res=res)
        err, bd = np.abs(got - want), L.bound(want, mag, K)
        print("K = %4d%s: worst err / bound %.3f, accumulation term used %.2f x 2^-24 sum|w x|" % (
            K, " + residual" if res else "", (err / bd).max(), L.accumulation_ratio(got, want, mag)))
        assert (err <= bd).all(), (K, res, float((err / bd).max()))
        if K == 27:        # the leading term is not loose: with u_h taken as 2^-12 the rounding to half alone breaks the bound at a short K
            assert (err > bd - 0.5 * L.U_H * np.abs(want) * (1 + 2.0 ** -8)).any()


@pytest.mark.parametrize("K", [36, 288, 2304])
def test_float32_variant_stays_inside_its_bound(K):
    got, want, mag = _emulate(K, np.random.RandomState(K + 1), out_f32=True)
    err, bd = np.abs(got - want), L.bound(want, mag, K, out_f32=True)
    print("float32 K = %4d: worst err / bound %.3f" % (K, (err / bd).max()))
    assert (err <= bd).all()


def test_planted_omissions_fall_outside_the_bound():
    """A dropped 3x3 tap (32 of K = 288 inputs), and the last 16 input channels of an 80-channel input dropped -- in a 1x1 layer (16
    of K = 80) and as the K tail of a 3x3 layer (the last 16 of K = 720, the bug of the record): each puts more than half of the
    elements outside the bound, so the bound tells these bugs from rounding."""
    rs = np.random.RandomState(7)
    for name, K, drop in (("one 3x3 tap of 32 channels", 288, slice(4 * 32, 5 * 32)), ("channels 64-79 of a 1x1 80 -> 80", 80, slice(64, 80)),
                          ("the last 16 of K = 720", 720, slice(704, 720)), ("the last 16 of K = 2304", 2304, slice(2288, 2304))):
        keep = np.ones(K, bool)
        keep[drop] = False
        got, want, mag = _emulate(K, rs, keep=keep)
        outside = float((np.abs(got - want) > L.bound(want, mag, K)).mean())
        print("dropped %s: %.1f %% of the elements outside the bound" % (name, 100 * outside))
        assert outside > 0.5, (name, outside)


def test_pools_and_upsample_are_the_oracles():
    import torch
    import torch.nn.functional as F
    x = np.random.RandomState(3).standard_normal((2, 6, 20, 8))
    for H in (1, 2, 6):                                      # a 1-row map included
        t = torch.from_numpy(x[:, :H].transpose(0, 3, 1, 2).copy())
        y1 = F.max_pool2d(t, 5, 1, 2)
        y2 = F.max_pool2d(y1, 5, 1, 2)
        y3 = F.max_pool2d(y2, 5, 1, 2)
        want = torch.cat([y1, y2, y3], 1).numpy().transpose(0, 2, 3, 1)
        assert np.array_equal(L.pools_want(x[:, :H]), want)
        assert np.array_equal(L.upsample_want(x[:, :H]), F.interpolate(t, scale_factor=2, mode="nearest").numpy().transpose(0, 2, 3, 1))


def test_chained_per_op_reference_is_the_oracles_network():
    """The float64 per-op reference, chained with the float32 parameters (no rounding anywhere), against oracle/yolo_ref.py's float32
    network: every named map and the six head outputs within 1e-5 of the map's maximum -- two restatements of one network."""
    import torch
    from oracle import yolo_ref as R
    params = R.random_params(0)
    x = R.preprocess(L.case_frames("C")[1])                  # [3, 192, 640]
    with torch.no_grad():
        f = R.build_model(params).features(torch.from_numpy(x)[None])
    bufs = L.run_chain(params, x.transpose(1, 2, 0)[None])
    maps = [(k, f[k], L.NAMED[k]) for k in L.NAMED]
    for i, (b, c) in enumerate(f["head"]):
        maps += [("head %d box" % i, b, ("h%d.box" % i, 0, 64)), ("head %d cls" % i, c, ("h%d.cls" % i, 0, 80))]
    for key, t, (buf, off, c) in maps:
        want, have = t[0].numpy().transpose(1, 2, 0), bufs[buf][0, :, :, off:off + c]
        assert have.shape == want.shape, key
        rel = np.abs(have - want).max() / np.abs(want).max()
        assert rel < 1e-5, (key, rel)


def test_float32_folding_gives_the_half_weights_of_float64_folding():
    """fold_bn's arithmetic (scale = g / sqrt(var + 1e-3), w scale) in float32, rounded to half, against the same in float64 rounded to
    half.  The float32 result is within 4 float32 roundings (2^-22 relative) of the float64 one, so the two halves differ only where
    the value lies that close to the midpoint of two halves -- by one half ulp, and in at most 2 * 2^-22 / 2^-11 = 2^-10 of the
    elements if values are spread evenly between midpoints (asserted with a factor 2 to spare)."""
    from oracle import yolo_ref as R
    params = R.random_params(0)
    n = differ = 0
    for (w32, b32), (w64, b64) in zip(L.fold(params, np.float32), L.fold(params, np.float64)):
        assert w32.dtype == np.float32 and np.abs(b32 - b64).max() <= 2.0 ** -22 * (np.abs(b64).max() + 1)
        h32, h64 = w32.astype(np.float16), w64.astype(np.float16)
        ne = h32 != h64
        if ne.any():
            step = np.abs(h32[ne].view(np.int16).astype(np.int32) - h64[ne].view(np.int16).astype(np.int32))
            assert (step == 1).all()                         # neighbouring halves of one sign
            assert (np.abs(w32[ne].astype(np.float64) - w64[ne]) <= 2.0 ** -22 * np.abs(w64[ne])).all()
        n, differ = n + ne.size, differ + int(ne.sum())
    print("float32 against float64 folding: %d of %d half weights differ, each by one half ulp" % (differ, n))
    assert differ <= n * 2.0 ** -9


@pytest.mark.parametrize("case", ["A", "B", "C", "E"])       # (D's images are A's shape with other noise)
def test_every_op_of_a_case_has_outputs_the_bound_can_judge(case):
    """The condition tests/test_gpu_yolo_layers.py asserts on the device's maps, on the host chain first: for every op fewer than half
    of the elements in half's subnormal range, at least 1 % above a tenth of the map's maximum."""
    from oracle import yolo_ref as R
    frames = L.case_frames(case)[:1 if case == "E" else 2]
    x = np.stack([R.preprocess(fr).transpose(1, 2, 0) for fr in frames])
    assert x.shape[1:3] == L.CASES[case]["net"]
    bad = []

    def on_op(k, op, want, mag):
        small, large = L.nonvacuous(want)
        if not (small < 0.5 and large >= 0.01):
            bad.append((k, op["kind"], op["out"], small, large))
    L.run_chain(R.random_params(0), x, half=True, on_op=on_op)
    assert not bad, bad
