"""YOLO-mode detector: MFMA conv path vs the PyTorch-CPU fp32 oracle (parity unpinned: ultralytics absent)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from multimodal_autonomous_driving_perception_and_planning_amd.perception import yolo as Y
    from oracle import yolo_ref as R
    from oracle.lane_ref import synthetic_frame
    assert Y.conv_specs() == R.conv_specs() and np.array_equal(Y.random_params(3), R.random_params(3))
    frame = synthetic_frame(720, 1280, 0, 0)
    params = R.random_params(0)
    net = R.build_model(params)
    with torch.no_grad():
        feats = net.features(torch.from_numpy(R.preprocess(frame))[None])
    model = Y.YoloV8n("random:0", keep_logits=True)      # the logit-level tests need the float32 head outputs
    got = model.detect(frame)
    return Y, R, frame, feats, model, got


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def test_preprocess_and_feature_maps(setup):
    Y, R, frame, feats, model, _ = setup
    assert model.dims() == (384, 640, 5040)
    t0 = model.tensor(0)                       # RGB inside a one-pixel frame of zeros (the stem's padding)
    assert t0.shape == (386, 642, 3) and not t0[0].any() and not t0[-1].any() and not t0[:, 0].any() and not t0[:, -1].any()
    x = t0[1:-1, 1:-1].transpose(2, 0, 1)
    assert np.abs(x - R.preprocess(frame)).max() <= 2 ** -11         # half rounding of values in [0,1]
    for tid, key in ((1, "l1"), (2, "l2"), (4, "l4"), (6, "l6"), (8, "l8"), (9, "l9"), (12, "l12"), (15, "p3"),
                     (18, "p4"), (21, "p5")):
        want = feats[key][0].numpy().transpose(1, 2, 0)
        have = model.tensor(tid)
        assert have.shape == want.shape, key
        print("feature map %-4s max err / max |x| = %.5f   mean err / mean |x| = %.5f" % (
            key, _rel(have, want), np.abs(have - want).mean() / np.abs(want).mean()))
        assert _rel(have, want) < 0.004, (key, _rel(have, want))      # measured <= 0.0015 (half activations/weights, fp32 accumulate; bf16 gave 0.06)
        assert np.abs(have - want).mean() < 0.0015 * np.abs(want).mean() + 1e-5, key   # measured <= 0.0008


def test_feature_maps_at_a_resolution_with_partial_tiles(setup):
    """600x800 input -> 480x640 network input: the maps are 120x160, 60x80, 30x40, 15x20, so the persistent kernels' 16- and
    8-row tiles, the stride-2 kernel's 17x33 patches and the fused block's 16x16 tiles all end in partial tiles, and the
    last stride-2 layer halves an odd height.  Same tolerances as at 720p."""
    import torch
    Y, R, frame, feats, model, _ = setup
    rs = np.random.RandomState(5)
    fr = rs.randint(0, 256, (600, 800, 3)).astype(np.uint8)
    fr[200:420, 100:500] = (40, 180, 90)
    net = R.build_model(R.random_params(0))
    with torch.no_grad():
        f = net.features(torch.from_numpy(R.preprocess(fr))[None])
    m = Y.YoloV8n("random:0", keep_logits=True)
    m.detect(fr)
    assert m.dims()[:2] == (480, 640)
    for tid, key in ((1, "l1"), (2, "l2"), (4, "l4"), (6, "l6"), (8, "l8"), (9, "l9"), (12, "l12"), (15, "p3"), (18, "p4"), (21, "p5")):
        want, have = f[key][0].numpy().transpose(1, 2, 0), m.tensor(tid)
        assert have.shape == want.shape, key
        assert _rel(have, want) < 0.004, (key, _rel(have, want))
        assert np.abs(have - want).mean() < 0.0015 * np.abs(want).mean() + 1e-5, key
    for i, (b, c) in enumerate(f["head"]):
        assert _rel(m.tensor(100 + 2 * i), b[0].numpy().transpose(1, 2, 0)) < 0.001
        assert _rel(m.tensor(101 + 2 * i), c[0].numpy().transpose(1, 2, 0)) < 0.001
    m.close()


def test_head_logits_and_decode(setup):
    Y, R, frame, feats, model, _ = setup
    for i, (b, c) in enumerate(feats["head"]):
        hb, hc = model.tensor(100 + 2 * i), model.tensor(101 + 2 * i)
        rb, rc = _rel(hb, b[0].numpy().transpose(1, 2, 0)), _rel(hc, c[0].numpy().transpose(1, 2, 0))
        print("head level %d: box logits %.5f, class logits %.5f (max err / max |x|)" % (i, rb, rc))
        assert rb < 0.001 and rc < 0.001                                # measured <= 0.0003 (bf16: 0.08)


def test_nms_matches_oracle_on_device_candidates(setup):
    """NMS is checked on the oracle's own decode of the DEVICE logits, so rounding noise does not decide selections."""
    import torch
    Y, R, frame, feats, model, got = setup
    head = []
    for i in range(3):
        hb, hc = model.tensor(100 + 2 * i), model.tensor(101 + 2 * i)
        head.append((torch.from_numpy(hb.transpose(2, 0, 1).copy())[None], torch.from_numpy(hc.transpose(2, 0, 1).copy())[None]))
    xyxy, conf, cls = R.decode(head)
    keep = R.nms(xyxy, conf, cls)
    boxes, gconf, gcls = got
    assert len(boxes) == len(keep) <= 300
    want = R.scale_boxes(xyxy[keep], 720, 1280)
    # identical selection except where float32 exp/softmax differences reorder near-equal confidences
    same = np.abs(boxes - want).max(axis=1) < 0.5
    assert same.mean() > 0.9, same.mean()
    assert np.all(np.diff(gconf) <= 1e-6)
    assert np.abs(np.sort(gconf)[::-1][:50] - np.sort(conf[keep])[::-1][:50]).max() < 1e-3
    assert boxes.min() >= 0 and boxes[:, [0, 2]].max() <= 1280 and boxes[:, [1, 3]].max() <= 720


def test_end_to_end_detections_match_fp32_oracle(setup, tmp_path):
    """ObjectDetector(mode="yolo").detect() -- and the 64-frame batch path bench config3 runs -- against the fp32
    restatement run END TO END on its own logits (decode, NMS, scale_boxes, int()).

    Greedy NMS over the frame-sized, heavily overlapping boxes a random network emits is a cascade: one swap of two
    near-tied confidences changes every later decision, and the fp32 restatement ITSELF flips 10-57 % of its boxes when
    its class logits are perturbed by the half-precision network's logit error.  A flip-rate
    allowance therefore cannot tell "NMS cascade" from "wrong box kept".  What is asserted instead, per frame:

    1. EXACT, on the production path (no logits kept): the oracle's threshold + sort + NMS + scale_boxes + int() applied
       to the DEVICE's per-anchor candidates give the device's detections box for box -- any error in the threshold, the
       (confidence desc, anchor asc) order, the float32 IoU test, max_det, scale_boxes or the truncation shows here,
       for every frame and both parameter sets;
    2. the candidates themselves: every anchor's box within 0.05 px and confidence within 2e-3 / 1e-4 of the fp32
       restatement's (the only place the network's arithmetic enters), logits within 0.001 max|x|;
    3. the SET statement on the fp32 restatement's own detections: with eps = the device's measured logit error, the
       oracle's post-processing is re-run on its logits perturbed by uniform +-eps noise (24 trials); every box that ALL
       runs keep (its fate does not depend on rounding noise) must be kept by the device, and every device box must be
       kept by SOME run, +-1 px, same class.  The flip rate is printed as a diagnostic only.

    Two parameter sets.  "spread": the random network with the class convolutions rescaled so that confidences spread
    over (0.01, 0.85) and ~210 of 5040 anchors pass the 0.25 filter -- the regime a trained detector works in.
    "random:0" (BASELINE config 3's plain random init): all 5040 confidences lie within 0.03 of each other with a median
    gap of 6.5e-7 between neighbours in the sorted list."""
    import torch
    from src.perception import ObjectDetector
    from tests._util import match_detections, selection_sets, spread_params
    from tools.yolo_e2e import candidate_stats, oracle_detections
    Y, R, frame, feats, model, got = setup
    from oracle.lane_ref import synthetic_frame
    frames = [frame] + [synthetic_frame(720, 1280, s, f) for s, f in ((3, 11), (6, 40), (1, 5), (2, 77))]
    frames.append(np.full((720, 1280, 3), 128, np.uint8))
    TRIALS = 24

    def post(head):
        xyxy, conf, cls = R.decode(head)
        keep = R.nms(xyxy, conf, cls)
        return np.trunc(R.scale_boxes(xyxy[keep], 720, 1280)), conf[keep], cls[keep]

    def exact_on_device_candidates(m, fr):
        """statement 1: m is a production-mode model (decode in the head's epilogue, no logits)"""
        gb, gc, gk = m.detect(fr)
        cb, cc, ck = m.tensor(110)[0], m.tensor(111)[0, :, 0], m.tensor(112)[0, :, 0]
        keep = R.nms(cb, cc, ck)
        assert len(keep) == len(gb)
        assert np.array_equal(R.scale_boxes(cb[keep], 720, 1280), gb), "kept boxes differ from the oracle's NMS on the same candidates"
        assert np.array_equal(cc[keep], gc) and np.array_equal(ck[keep], gk)
        return gb, gc, gk

    def logit_error(probe, f):
        eb = ec = 0.0
        for i, (b, c) in enumerate(f["head"]):
            hb, hc = probe.tensor(100 + 2 * i), probe.tensor(101 + 2 * i)
            db, dc = np.abs(hb - b[0].numpy().transpose(1, 2, 0)).max(), np.abs(hc - c[0].numpy().transpose(1, 2, 0)).max()
            assert db < 0.001 * float(b.abs().max()) + 1e-6 and dc < 0.001 * float(c.abs().max()) + 1e-6
            eb, ec = max(eb, float(db)), max(ec, float(dc))
        return eb, ec

    def set_statement(tag, k, f, eb, ec, gb, gk, rs, trials=TRIALS, outside_allowed=0):
        runs = [post(f["head"])]
        for trial in range(trials):
            hd = [(b + torch.from_numpy(rs.uniform(-eb, eb, tuple(b.shape)).astype(np.float32)),
                   c + torch.from_numpy(rs.uniform(-ec, ec, tuple(c.shape)).astype(np.float32))) for b, c in f["head"]]
            runs.append(post(hd))
        sets = [(b, kk) for b, _, kk in runs]
        core_missing, outside, n_core, _ = selection_sets(np.trunc(gb), gk, sets, 1.0)
        wb, wk = sets[0]
        pairs, miss, extra, worst = match_detections(np.trunc(gb), gk, wb, wk, 1.0)
        print("%s frame %d: oracle %d / device %d boxes, %d matched (flip rate %.3f, diagnostic), stable core %d, "
              "core boxes missing %d, device boxes outside the union of %d runs: %d; logit error box %.2g cls %.2g"
              % (tag, k, len(wb), len(gb), len(pairs), (len(miss) + len(extra)) / max(1, len(gb) + len(wb)), n_core,
                 core_missing, len(runs), outside, eb, ec))
        assert core_missing == 0 and outside <= outside_allowed, (tag, k, core_missing, outside)
        assert worst <= 1.0
        return n_core

    # ---- "spread" parameters ----------------------------------------------------------------------------------
    params = spread_params(0)
    path = str(tmp_path / "spread.npy")
    np.save(path, params)
    net = R.build_model(params)
    det = ObjectDetector(mode="yolo", model_path=path)
    assert det.mode == "yolo"
    probe = Y.YoloV8n(path, keep_logits=True)          # same network with the float32 logits kept: measures the logit error
    prod = Y.YoloV8n(path)                             # the production path
    rs = np.random.RandomState(0)
    class_path, n_core_total, n_want_total = [], 0, 0
    for k, fr in enumerate(frames):
        wb, wc, wk, f = oracle_detections(R, net, fr, torch)
        out = det.detect(fr)
        gb = np.array([d.bbox for d in out], np.float64).reshape(-1, 4)
        gk = np.array([d.class_id for d in out], np.int32)
        class_path.append((gb, gk))
        pb, pc, pk = exact_on_device_candidates(prod, fr)
        assert np.array_equal(np.trunc(pb), gb) and np.array_equal(pk, gk)        # the class returns int()-truncated boxes of the same path
        qb, _, qk = probe.detect(fr)
        assert np.array_equal(qb, pb) and np.array_equal(qk, pk)                   # keeping the logits changes nothing
        eb, ec = logit_error(probe, f)
        n_core_total += set_statement("spread", k, f, eb, ec, gb, gk, rs)
        n_want_total += len(wb)
    assert n_want_total > 150 and n_core_total > 20, (n_want_total, n_core_total)     # the statements are about something
    # the 64-frame batch path (bench config3): image b of the batch gives exactly the class path's detections of that frame
    B = 64
    batched = Y.YoloV8n(path, batch=B)
    batched._prepare(720, 1280)
    batched._frames.copy_(torch.as_tensor(np.stack([frames[b % len(frames)] for b in range(B)])))
    batched.forward_device(batched._frames)
    torch.cuda.synchronize()
    n = batched._n.cpu().numpy()
    box, cls = batched._box.cpu().numpy(), batched._cls.cpu().numpy()
    for b in range(B):
        gb, gk = class_path[b % len(frames)]
        assert n[b] == len(gb) and np.array_equal(np.trunc(box[b, :n[b]]), gb) and np.array_equal(cls[b, :n[b]], gk), b
    batched.close()
    prod.close()
    # per-anchor candidates under the spread parameters
    for fr in frames[:3]:
        st = candidate_stats(probe, fr, R, net, torch)
        assert st["box_max_px"] < 0.05 and st["conf_max"] < 2e-3 and st["class_flips"] <= 10, st
    probe.close()
    # ---- plain random init (BASELINE config 3's parameters): the same three statements -------------------------
    net0 = R.build_model(R.random_params(0))
    prod0 = Y.YoloV8n("random:0")
    for k, fr in enumerate(frames[:3]):
        st = candidate_stats(model, fr, R, net0, torch)
        assert st["box_max_px"] < 0.05 and st["conf_max"] < 1e-4 and st["class_flips"] == 0, st
        gb, gc, gk = exact_on_device_candidates(prod0, fr)
        with torch.no_grad():
            f = net0.features(torch.from_numpy(R.preprocess(fr))[None])
        model.detect(fr)
        eb, ec = logit_error(model, f)
        # 300 kept boxes out of ~1700 walked, many of them kept in only a few per cent of the outcomes: a finite number of runs
        # cannot cover every box of one particular outcome, so 1 % of the device's boxes may lie outside the union of 96 runs
        # (measured: 3 of 300 outside 24 runs); the stable core must be kept without exception
        set_statement("random:0", k, f, eb, ec, gb, gk, rs, trials=96, outside_allowed=len(gb) // 100)
    prod0.close()


def test_fused_kernels_are_bit_identical_to_their_separate_launches(setup, monkeypatch):
    """front_fused_kernel (2:1 letterbox + stem + layer 1 in one launch), c2f16_fused_kernel (layer 2: cv1, 3x3,
    3x3 + shortcut, cv2 in one launch) and the 32-channel blocks at P3 (layer 4: c2f32_head_kernel + c2f32_tail_kernel for
    its six convolutions; layer 15: cv1 + c2f32_tail_kernel) and the virtual Upsample + Concat in front of layers 12 and 15
    (no upsample launch: cv1 fetches the half-resolution source itself) against the separate launches (AVHOT_YOLO_NO_FUSE, read
    per forward): every element of the outputs of layers 1, 2, 4, 12 and 15, borders included, on frames with different content,
    in a batch large enough that persistent workgroups walk more than one tile -- and the detections at the end."""
    import torch
    Y, R, frame, feats, model, _ = setup
    from oracle.lane_ref import synthetic_frame
    rs = np.random.RandomState(11)
    frames = [frame] + [synthetic_frame(720, 1280, s, f) for s, f in ((6, 40), (2, 77))] + [np.full((720, 1280, 3), 255, np.uint8)]
    frames.append(rs.randint(0, 256, (720, 1280, 3)).astype(np.uint8))          # noise: every pixel of every halo matters
    frames = frames * 4                                  # 20 images: 2400 front tiles / 1200 layer-2 tiles on 512 persistent workgroups, 300 P3 tiles on 256
    m = Y.YoloV8n("random:0", batch=len(frames))
    m._prepare(720, 1280)
    m._frames.copy_(torch.as_tensor(np.stack(frames)))

    def run():
        m.forward_device(m._frames)
        torch.cuda.synchronize()
        return (m.tensor(1, image=None), m.tensor(2, image=None), m._n.cpu().numpy().copy(), m._box.cpu().numpy().copy(),
                m._conf.cpu().numpy().copy(), m.tensor(4, image=None), m.tensor(15, image=None), m.tensor(12, image=None))
    fused = run()
    monkeypatch.setenv("AVHOT_YOLO_NO_FUSE", "1")
    unfused = run()
    monkeypatch.delenv("AVHOT_YOLO_NO_FUSE")
    assert fused[0].shape == (len(frames), 96, 160, 32) and fused[0].any() and fused[1].shape == (len(frames), 96, 160, 32) and fused[1].any()
    assert fused[5].shape == (len(frames), 48, 80, 64) and fused[5].any() and fused[6].shape == (len(frames), 48, 80, 64) and fused[6].any()
    assert fused[7].shape == (len(frames), 24, 40, 128) and fused[7].any()
    # (layers 12 and 15 also cover the virtual Upsample + Concat: their cv1 reads the half-resolution source directly)
    for k, name in ((0, "layer 1"), (1, "layer 2"), (5, "layer 4"), (7, "layer 12"), (6, "layer 15")):
        assert np.array_equal(fused[k].view(np.uint32), unfused[k].view(np.uint32)), (name, int((fused[k] != unfused[k]).sum()))
    assert np.array_equal(fused[2], unfused[2]) and np.array_equal(fused[3], unfused[3]) and np.array_equal(fused[4], unfused[4])
    # the keep_logits model (three launches, network input and stem map kept) gives the same layer-1 map as the production path
    model.detect(frames[4])
    assert np.array_equal(model.tensor(1).view(np.uint32), fused[0][4].view(np.uint32))
    m.close()


def test_cin80_layers_equal_generic_kernels(setup, monkeypatch):
    """The 80-channel layers of the head's class branches (3x3 64/128/256 -> 80 have cin <= 256; 3x3 80 -> 80 and 1x1 80 -> 80
    have a partial 32-channel chunk) run their last 16 input channels as a zero-padded K = 32 MFMA step in the weight-stationary
    kernels.  AVHOT_CONV_GENERIC80 (read per forward) sends exactly those layers through conv_lds_kernel / conv_mfma_kernel,
    whose padded K is the same arithmetic in the same order: the class logits of all three levels must be equal bit for bit
    (this pins the replacement of the K = 16 MFMA tail, which could read a stale accumulator behind a K = 32 MFMA)."""
    import torch
    Y, R, frame, feats, model, _ = setup
    from oracle.lane_ref import synthetic_frame
    frames = [frame, synthetic_frame(720, 1280, 6, 40), np.full((720, 1280, 3), 200, np.uint8), synthetic_frame(720, 1280, 2, 77)] * 2
    m = Y.YoloV8n("random:0", batch=len(frames), keep_logits=True)
    m._prepare(720, 1280)
    m._frames.copy_(torch.as_tensor(np.stack(frames)))

    def cls_logits():
        m.forward_device(m._frames)
        return [m.tensor(101 + 2 * i, image=None).copy() for i in range(3)]
    ws = cls_logits()
    monkeypatch.setenv("AVHOT_CONV_GENERIC80", "1")
    generic = cls_logits()
    monkeypatch.delenv("AVHOT_CONV_GENERIC80")
    for i in range(3):
        assert ws[i].shape[0] == len(frames) and ws[i].shape[3] == 80 and np.isfinite(ws[i]).all() and ws[i].any()
        assert np.array_equal(ws[i].view(np.uint32), generic[i].view(np.uint32)), (i, int((ws[i] != generic[i]).sum()))
    m.close()


def test_fused_decode_equals_decode_kernel(setup):
    """The head's last convolutions decode in their epilogue (DFL expectation per lane group, first-maximum class across
    lane groups); decode_kernel does the same from the float32 logits.  With keep_logits both run: every anchor's box,
    confidence and class must be equal bit for bit, for a batch whose frames differ, and a model without kept logits (the
    production path: no logits written at all) must return the same detections."""
    import torch
    Y, R, frame, feats, model, _ = setup
    from oracle.lane_ref import synthetic_frame
    frames = [frame, synthetic_frame(720, 1280, 6, 40), np.full((720, 1280, 3), 200, np.uint8), synthetic_frame(720, 1280, 2, 77)]
    out = {}
    for keep in (True, False):
        m = Y.YoloV8n("random:0", batch=len(frames), keep_logits=keep)
        m._prepare(720, 1280)
        m._frames.copy_(torch.as_tensor(np.stack(frames)))
        m.forward_device(m._frames)
        torch.cuda.synchronize()
        out[keep] = (m._n.cpu().numpy().copy(), m._box.cpu().numpy().copy(), m._conf.cpu().numpy().copy(), m._cls.cpu().numpy().copy())
        if keep:
            for a_id, b_id in ((110, 120), (111, 121), (112, 122)):
                a, b = m.tensor(a_id, image=None), m.tensor(b_id, image=None)
                assert a.shape == b.shape and a.shape[0] == len(frames) and a.shape[2] == 5040
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (a_id, int((a != b).sum()))
            assert np.isfinite(m.tensor(110, image=None)).all() and (m.tensor(111, image=None) > 0).all()
        m.close()
    n = out[True][0]
    assert np.array_equal(n, out[False][0]) and n.min() > 0
    for b in range(len(frames)):
        for k in (1, 2, 3):
            assert np.array_equal(out[True][k][b, :n[b]], out[False][k][b, :n[b]]), (b, k)


def test_object_detector_yolo_mode(setup, tmp_path):
    import torch
    from src.perception import ObjectDetector
    Y, R, frame, feats, model, got = setup
    # a YOLOv8n state_dict file with ultralytics' key names drops in as model_path (detector.py:77-84, demo.py:41)
    pt = str(tmp_path / "yolov8n_state_dict.pt")
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in Y.state_dict_from_params(R.random_params(0)).items()}, pt)
    from_sd = ObjectDetector(mode="yolo", model_path=pt)
    assert from_sd.mode == "yolo"
    out_sd = from_sd.detect(frame)
    assert [d.bbox for d in out_sd] == [tuple(int(v) for v in b) for b in got[0]]
    det = ObjectDetector(mode="yolo", model_path="random:0")
    assert det.mode == "yolo" and det.model is not None
    out = det.detect(frame)
    assert len(out) == len(got[0]) and det.frame_count == 1
    d0 = out[0]
    assert d0.bbox == tuple(int(v) for v in got[0][0]) and d0.class_name == Y.COCO_NAMES[d0.class_id]
    assert isinstance(d0.bbox[0], int) and 0.25 < d0.confidence <= 1.0
    # a missing checkpoint degrades to simulated mode like the reference without ultralytics (detector.py:79-84)
    fb = ObjectDetector(mode="yolo", model_path="yolov8n.pt")
    assert fb.mode == "simulated" and 3 <= len(fb.detect(frame)) <= 7


def test_batch_of_different_frames_matches_single_image_runs(setup):
    """bench config3 runs 64 frames per launch: every image of a batch must come out exactly as it does alone
    (same kernels, per-image tiles; nothing may leak across the image index)."""
    import torch
    Y, R, frame, feats, model, got = setup
    from oracle.lane_ref import synthetic_frame
    frames = [frame, synthetic_frame(720, 1280, 3, 11), np.full((720, 1280, 3), 128, np.uint8), synthetic_frame(720, 1280, 6, 40),
              synthetic_frame(720, 1280, 1, 5)]
    B = len(frames)
    batched = Y.YoloV8n("random:0", batch=B)
    batched._prepare(720, 1280)
    batched._frames.copy_(torch.as_tensor(np.stack(frames)))
    batched.forward_device(batched._frames)
    torch.cuda.synchronize()
    n = batched._n.cpu().numpy()
    box, conf, cls = batched._box.cpu().numpy(), batched._conf.cpu().numpy(), batched._cls.cpu().numpy()
    for b in range(B):
        sb, sc, sk = model.detect(frames[b])
        assert n[b] == len(sc) > 0, b
        assert np.array_equal(box[b, :n[b]], sb) and np.array_equal(conf[b, :n[b]], sc) and np.array_equal(cls[b, :n[b]], sk), b
    assert not np.array_equal(box[0, :8], box[1, :8])            # the frames really differ
    batched.close()


def test_unaligned_frame_pointer_gives_the_same_detections(setup):
    """The 2:1 letterbox kernels (front_fused_kernel, preprocess2_kernel) read dwords and need a 4-byte aligned frame pointer; the
    alignment is the one thing a forward decides per call.  The same frames at an odd address go through preprocess_kernel +
    stem + layer 1 and must give the same detections bit for bit."""
    import torch
    Y, R, frame, feats, model, got = setup
    from oracle.lane_ref import synthetic_frame
    frames = np.stack([frame, synthetic_frame(720, 1280, 3, 11)])
    m = Y.YoloV8n("random:0", batch=2)
    m._prepare(720, 1280)
    m._frames.copy_(torch.as_tensor(frames))
    assert m._frames.data_ptr() % 4 == 0
    m.forward_device(m._frames)
    torch.cuda.synchronize()
    want = [t.cpu().numpy().copy() for t in (m._n, m._box, m._conf, m._cls)]
    assert want[0].min() > 0
    raw = torch.empty(frames.size + 1, dtype=torch.uint8, device=m._frames.device)
    odd = raw[1:].view(frames.shape)
    odd.copy_(torch.as_tensor(frames))
    assert odd.data_ptr() % 4 == 1
    m.forward_device(odd)
    torch.cuda.synchronize()
    for a, b in zip(want, (m._n, m._box, m._conf, m._cls)):
        assert np.array_equal(a, b.cpu().numpy())
    m.close()


def test_perception_loop_step_matches_per_frame_paths(setup):
    """bench config3's step -- frames generated on the device, lane chain forked beside the detector, join -- gives
    per camera what the per-frame paths give: the oracle's lanes on the oracle's frame (EMA over the steps) and the
    single-image detector's boxes."""
    import torch
    Y, R, frame, feats, model, got = setup
    from multimodal_autonomous_driving_perception_and_planning_amd.pipeline import PerceptionLoop
    from oracle.lane_ref import LaneRef, synthetic_frame
    S, h, w = 3, 720, 1280
    loop = PerceptionLoop(n_streams=S, h=h, w=w)
    refs = [LaneRef() for _ in range(S)]
    seen = []
    for step in range(3):
        loop.step(sync=True)
        torch.cuda.synchronize()
        fr = loop.frames.cpu().numpy()
        info, poly, pts = loop.info.cpu().numpy(), loop.poly.cpu().numpy(), loop.pts.cpu().numpy()
        n, box = loop.det_n.cpu().numpy(), loop.det_box.cpu().numpy()
        for s in range(S):
            assert np.array_equal(fr[s], synthetic_frame(h, w, s, step)), (step, s)
            want = refs[s].detect(fr[s])
            assert info[s, 4] == len(want["segments"]), (step, s)
            for side, exp in ((0, want["left"]), (1, want["right"])):
                assert bool(info[s, side]) == (exp is not None), (step, s, side)
                if exp is not None:
                    np.testing.assert_allclose(poly[s, side], exp[2], rtol=1e-6, atol=1e-6)
                    assert np.abs(pts[s, side] - exp[0]).max() <= 1
            sb, sc, sk = model.detect(fr[s])
            assert n[s] == len(sc) and np.array_equal(box[s, :n[s]], sb), (step, s)
        seen.append((info.copy(), poly.copy(), pts.copy(), loop.conf.cpu().numpy(), n.copy(), box.copy()))
    # throughput variant: the Hough + fit half of the lane chain one step late -- same results, one step later
    loop2 = PerceptionLoop(n_streams=S, h=h, w=w)

    def lanes_equal(k):
        got = (loop2.info.cpu().numpy(), loop2.poly.cpu().numpy(), loop2.pts.cpu().numpy(), loop2.conf.cpu().numpy())
        return all(np.array_equal(a, b) for a, b in zip(got, seen[k][:4]))
    for step in range(3):
        loop2.step_deferred()
        loop2.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(loop2.det_n.cpu().numpy(), seen[step][4]) and np.array_equal(loop2.det_box.cpu().numpy(), seen[step][5])
        if step:
            assert lanes_equal(step - 1), step
    loop2.flush_lanes()
    loop2.synchronize()
    torch.cuda.synchronize()
    assert lanes_equal(2)
    # detector tail (decode + sort + NMS) deferred onto its own stream beside the next step's convolutions: same detections
    loop3 = PerceptionLoop(n_streams=S, h=h, w=w)
    loop3.defer_detector_tail(True)
    for step in range(3):
        loop3.step_deferred()
    loop3.flush_lanes()                     # also joins the detector's tail
    loop3.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(loop3.det_n.cpu().numpy(), seen[2][4]) and np.array_equal(loop3.det_box.cpu().numpy(), seen[2][5])


def test_two_to_one_preprocess_equals_generic_kernel(setup, monkeypatch):
    """1280x720 frames take the 2:1 letterbox kernel (two output pixels from 12 contiguous bytes of two rows); it must
    write exactly what the generic bilinear kernel writes."""
    Y, R, frame, feats, model, _ = setup
    model.detect(frame)                        # other tests ran other frames through this model
    fast = model.tensor(0).copy()
    monkeypatch.setenv("AVHOT_YOLO_GENERIC_PRE", "1")
    other = Y.YoloV8n("random:0")
    other.detect(frame)
    assert np.array_equal(other.tensor(0), fast)
    other.close()


def test_gemm_form_stride2_layers_equal_streaming_kernel(setup, monkeypatch):
    """The two cin = 128 stride-2 convolutions (layer 7: 128 -> 256 into P5; layer 19: 128 -> 128 in the neck) run as an LDS-tiled
    GEMM over flattened output pixels (conv_gemm128_kernel); AVHOT_CONV_NO_GEMM (read per forward) sends them through
    conv_mfma_kernel, whose K order, padding and epilogue are the same: their outputs and the detections must be the same bits
    (a batch whose 240-pixel maps do not fill the last 128-pixel tile: 5 images = 1200 pixels)."""
    import torch
    Y, R, frame, feats, model, _ = setup
    from oracle.lane_ref import synthetic_frame
    frames = [frame, synthetic_frame(720, 1280, 6, 40), np.full((720, 1280, 3), 200, np.uint8), synthetic_frame(720, 1280, 2, 77),
              np.random.RandomState(5).randint(0, 256, (720, 1280, 3)).astype(np.uint8)]
    m = Y.YoloV8n("random:0", batch=len(frames))
    m._prepare(720, 1280)
    m._frames.copy_(torch.as_tensor(np.stack(frames)))

    def run():
        m.forward_device(m._frames)
        torch.cuda.synchronize()
        return (m.tensor(7, image=None).copy(), m.tensor(19, image=None).copy(), m._n.cpu().numpy().copy(), m._box.cpu().numpy().copy(),
                m._conf.cpu().numpy().copy())
    gemm = run()
    monkeypatch.setenv("AVHOT_CONV_NO_GEMM", "1")
    stream = run()
    monkeypatch.delenv("AVHOT_CONV_NO_GEMM")
    assert gemm[0].shape == (len(frames), 12, 20, 256) and gemm[0].any() and gemm[1].shape == (len(frames), 12, 20, 128) and gemm[1].any()
    for k in range(2):
        assert np.array_equal(gemm[k].view(np.uint32), stream[k].view(np.uint32)), (k, int((gemm[k] != stream[k]).sum()))
    assert np.array_equal(gemm[2], stream[2]) and np.array_equal(gemm[3], stream[3]) and np.array_equal(gemm[4], stream[4])
    m.close()


def test_gemm_form_1x1_layers_equal_weight_stationary_kernels(setup, monkeypatch):
    """conv_gemm128_kernel also takes the 1 x 1 convolutions with cin a multiple of 64 and cout of 128 (cv1 / cv2 of the P4 / P5 blocks,
    SPPF); AVHOT_CONV_NO_GEMM_1X1 (read per forward) sends them through conv1x1_ws_kernel / conv_lds_kernel instead -- same chunk
    order, same epilogue.  The outputs of the blocks they sit in (layers 6, 8, 9, 12, 18, 21) and the detections must be the same bits."""
    import torch
    Y, R, frame, feats, model, _ = setup
    from oracle.lane_ref import synthetic_frame
    frames = [frame, synthetic_frame(720, 1280, 6, 40), np.full((720, 1280, 3), 200, np.uint8), synthetic_frame(720, 1280, 2, 77),
              np.random.RandomState(5).randint(0, 256, (720, 1280, 3)).astype(np.uint8)]
    m = Y.YoloV8n("random:0", batch=len(frames))
    m._prepare(720, 1280)
    m._frames.copy_(torch.as_tensor(np.stack(frames)))

    def run():
        m.forward_device(m._frames)
        torch.cuda.synchronize()
        return [m.tensor(t, image=None).copy() for t in (6, 8, 9, 12, 18, 21)] + [m._n.cpu().numpy().copy(), m._box.cpu().numpy().copy(),
                                                                                 m._conf.cpu().numpy().copy()]
    gemm = run()
    monkeypatch.setenv("AVHOT_CONV_NO_GEMM_1X1", "1")
    base = run()
    monkeypatch.delenv("AVHOT_CONV_NO_GEMM_1X1")
    for k in range(6):
        assert base[k].any() and np.array_equal(base[k].view(np.uint32), gemm[k].view(np.uint32)), (k, int((base[k] != gemm[k]).sum()))
    for k in range(6, 9):
        assert np.array_equal(base[k], gemm[k])
    m.close()


def test_per_frame_call_as_one_graph_equals_the_eager_launches(setup, monkeypatch):
    """ObjectDetector(mode="yolo").detect(frame) -- one frame per call, demo.py:107 -- replays the whole forward (about 56 launches
    on two lanes + sort + NMS) as ONE captured hipGraph from its third call on.  Same kernels, same arguments: the detections of
    every frame must be those of the eager launches bit for bit, also when the thresholds change (a second graph) and when the
    frame size changes (graphs dropped with the handle)."""
    Y, R, frame, feats, _, _ = setup
    from oracle.lane_ref import synthetic_frame
    frames = [frame, synthetic_frame(720, 1280, 3, 9), np.random.RandomState(11).randint(0, 256, (720, 1280, 3)).astype(np.uint8),
              synthetic_frame(720, 1280, 6, 2)]
    monkeypatch.setenv("AVHOT_YOLO_NO_GRAPH", "1")
    eager = Y.YoloV8n("random:0")
    monkeypatch.delenv("AVHOT_YOLO_NO_GRAPH")
    graph = Y.YoloV8n("random:0")
    assert graph.use_graph and not eager.use_graph
    for rep in range(3):
        for i, fr in enumerate(frames):
            a, b = eager.detect(fr), graph.detect(fr)
            assert len(a[1]) > 0 and all(np.array_equal(x, y) for x, y in zip(a, b)), (rep, i)
    assert len(graph._graphs) == 1 and not eager._graphs
    a, b = eager.detect(frames[1], conf=0.3, iou=0.5), None
    for _ in range(3):
        b = graph.detect(frames[1], conf=0.3, iou=0.5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(graph._graphs) == 2
    small = synthetic_frame(480, 640, 1, 1)
    for _ in range(3):
        a, b = eager.detect(small), graph.detect(small)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(graph._graphs) == 1                       # the 720p graphs went with their handle
    eager.close(), graph.close()


def test_reference_precision_mode_matches_the_fp32_oracle(setup, tmp_path):
    """YoloV8n(precision="fp32"): the reference's own arithmetic (ultralytics runs torch float32, detector.py:103-123) -- float32
    tensors, weights and MFMA operands (v_mfma_f32_16x16x4_f32), one generic kernel per layer.  Against the PyTorch-CPU fp32
    restatement: network input exact, every tapped feature map and every head logit within 1e-5 of the map's maximum (float32
    sums in a different order), every anchor's box within 1e-3 px and confidence within 1e-5.  On the spread-confidence
    weights (the regime a trained detector works in) the detections are then SET-EQUAL to the oracle's own end-to-end result,
    frame by frame, without any perturbation allowance: same count, every box matched with the same class, +-1 px after int().
    The half-precision production path is compared with this mode too: its detections on its own candidates are already
    exact; here its logits are shown to sit within the stated 0.001 max|x| of the float32 DEVICE logits as well."""
    import torch
    from tests._util import match_detections, spread_params
    from tools.yolo_e2e import oracle_detections
    Y, R, frame, feats, model, _ = setup
    from oracle.lane_ref import synthetic_frame
    m32 = Y.YoloV8n("random:0", precision="fp32")
    m32.detect(frame)
    assert m32.precision == "fp32" and m32.dims() == (384, 640, 5040)
    t0 = m32.tensor(0)
    assert t0.shape == (384, 640, 3)
    assert np.abs(t0.transpose(2, 0, 1) - R.preprocess(frame)).max() <= 1e-7
    worst = 0.0
    for tid, key in ((1, "l1"), (2, "l2"), (4, "l4"), (6, "l6"), (8, "l8"), (9, "l9"), (12, "l12"), (15, "p3"), (18, "p4"), (21, "p5")):
        want, have = feats[key][0].numpy().transpose(1, 2, 0), m32.tensor(tid)
        assert have.shape == want.shape, key
        worst = max(worst, _rel(have, want))
        assert _rel(have, want) < 1e-5, (key, _rel(have, want))
    for i, (b, c) in enumerate(feats["head"]):
        hb, hc = m32.tensor(100 + 2 * i), m32.tensor(101 + 2 * i)
        assert _rel(hb, b[0].numpy().transpose(1, 2, 0)) < 1e-5 and _rel(hc, c[0].numpy().transpose(1, 2, 0)) < 1e-5, i
        # the half-precision production path against the float32 device path (both this library's kernels)
        assert _rel(model.tensor(100 + 2 * i), hb) < 0.001 and _rel(model.tensor(101 + 2 * i), hc) < 0.001, i
    print("float32 mode: worst feature-map error / max |x| = %.2e" % worst)
    wb, wc, wk = R.decode(feats["head"])
    cb, cc, ck = m32.tensor(110)[0], m32.tensor(111)[0, :, 0], m32.tensor(112)[0, :, 0]
    assert np.abs(cb - wb).max() < 1e-3 and np.abs(cc - wc).max() < 1e-5 and (ck != wk).sum() <= 2
    m32.close()
    # end to end on the spread-confidence weights
    p = spread_params(0)
    path = str(tmp_path / "spread.npy")
    np.save(path, p)
    net = R.build_model(p)
    ms = Y.YoloV8n(path, precision="fp32")
    frames = [frame] + [synthetic_frame(720, 1280, s, f) for s, f in ((3, 11), (6, 40), (1, 5), (2, 77))]
    total = 0
    for k, fr in enumerate(frames):
        ob, oc, ok_, _ = oracle_detections(R, net, fr, torch)
        gb, gc, gk = ms.detect(fr)
        pairs, miss, extra, worst_px = match_detections(np.trunc(gb), gk, np.trunc(ob), ok_, 1.0)
        assert len(gb) == len(ob) > 0 and not miss and not extra, (k, len(gb), len(ob), miss, extra)
        assert max(abs(float(gc[j]) - float(oc[i])) for i, j in pairs) < 1e-5
        total += len(gb)
    print("float32 mode end to end: %d detections over %d frames, all matched" % (total, len(frames)))
    # and a batch: per-image results equal the single-image call's
    mb = Y.YoloV8n(path, precision="fp32", batch=3)
    mb._prepare(720, 1280)
    mb._frames.copy_(torch.as_tensor(np.stack(frames[:3])))
    mb.forward_device(mb._frames)
    torch.cuda.synchronize()
    n, box, conf, cls = mb._n.cpu().numpy(), mb._box.cpu().numpy(), mb._conf.cpu().numpy(), mb._cls.cpu().numpy()
    for b in range(3):
        sb, sc, sk = ms.detect(frames[b])
        assert n[b] == len(sc) and np.array_equal(box[b, :n[b]], sb) and np.array_equal(conf[b, :n[b]], sc) and np.array_equal(cls[b, :n[b]], sk), b
    ms.close(), mb.close()
