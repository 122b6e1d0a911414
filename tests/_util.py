import numpy as np


def kernel_path(n, C_, S, extra):
    """The kernel the planner entry points launch for S start states of n waypoints and C_ candidates, as the library's own launch
    plan names it (av_planner_launch_shape; needs no device): "block<G,NW>", "wave" or, when a path or list is given, "wave+extra"."""
    import ctypes as C
    import os
    from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    out = (C.c_int32 * 4)()
    nat.check(nat.lib().av_planner_launch_shape(n, C_, S, int(bool(extra)), out))
    if out[0]:
        return "wave+extra" if extra else "wave"
    return "block<%d,%d>" % (out[1], out[2])


def order_mismatch(cost_ref, order_ref, cost_got, order_got, rtol=1e-9):
    """Why a device ranking (cost_got, order_got) is not the oracle's (cost_ref, order_ref), or None when it is.

    Both orders are stable ascending sorts, order[r] = generation index of the r-th cheapest candidate.
      - candidates whose ORACLE costs are bit-equal (an exact tie) and whose DEVICE costs are bit-equal too must keep generation
        order in the device's ranking;
      - inside an exact oracle tie the device costs may differ only by a near-tie, |dc| <= rtol * |c|: the device's headings
        come from a polynomial atan2 within 2 ulp of libm's, and mirrored candidates that tie exactly through libm's roundings
        can come out an ulp apart (the device then ranks them by its own costs);
      - two candidates may swap places only when their oracle costs are a near-tie, 0 < |dc| <= rtol * |c|, or an exact tie
        the device split as above.
    """
    cost_ref, cost_got = np.asarray(cost_ref, np.float64), np.asarray(cost_got, np.float64)
    order_ref, order_got = np.asarray(order_ref), np.asarray(order_got)
    C = len(cost_ref)
    if sorted(order_got.tolist()) != list(range(C)):
        return "device order is not a permutation of 0..%d" % (C - 1)
    near = lambda a, b: np.abs(a - b) <= rtol * np.maximum(np.abs(a), np.abs(b))
    srt = np.sort(cost_ref, kind="stable")
    for v in np.unique(srt[:-1][srt[1:] == srt[:-1]]):
        grp = np.nonzero(cost_ref == v)[0]
        cg = cost_got[grp]
        if not near(cg.min(), cg.max()):
            return "oracle tie %s has device costs %s" % (grp.tolist(), cg.tolist())
    pos_ref, pos_got = np.empty(C, np.int64), np.empty(C, np.int64)
    pos_ref[order_ref], pos_got[order_got] = np.arange(C), np.arange(C)
    i, j = np.nonzero((pos_ref[:, None] < pos_ref[None, :]) & (pos_got[:, None] > pos_got[None, :]))   # swapped pairs
    tie = cost_ref[i] == cost_ref[j]
    bad = np.where(tie, cost_got[i] == cost_got[j], ~near(cost_ref[i], cost_ref[j]))
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        return "candidates %d and %d swapped (oracle costs %r, %r; device costs %r, %r)" % (
            i[k], j[k], cost_ref[i[k]], cost_ref[j[k]], cost_got[i[k]], cost_got[j[k]])
    return None


def orders_equivalent(cost_ref, order_ref, cost_got, order_got, rtol=1e-9):
    """order_mismatch(...) is None: exact ties in generation order unless the device split them by a near-tie, only near-ties
    swapped."""
    return order_mismatch(cost_ref, order_ref, cost_got, order_got, rtol) is None


def match_detections(got_box, got_cls, want_box, want_cls, px=1.0):
    """One-to-one matching of two detection sets: a pair matches when the classes agree and every box coordinate
    differs by at most `px`.  Greedy over the wanted boxes, best (smallest max |d|) partner first.
    -> (pairs [(i_want, j_got)], unmatched_want indices, unmatched_got indices, worst |d| over the pairs)."""
    got_box, want_box = np.asarray(got_box, np.float64).reshape(-1, 4), np.asarray(want_box, np.float64).reshape(-1, 4)
    used = np.zeros(len(got_box), bool)
    pairs, miss, worst = [], [], 0.0
    for i in range(len(want_box)):
        if len(got_box) == 0:
            miss.append(i)
            continue
        d = np.abs(got_box - want_box[i]).max(axis=1)
        d[used | (np.asarray(got_cls) != want_cls[i])] = np.inf
        j = int(np.argmin(d))
        if d[j] <= px:
            used[j] = True
            pairs.append((i, j))
            worst = max(worst, float(d[j]))
        else:
            miss.append(i)
    return pairs, miss, [int(j) for j in np.nonzero(~used)[0]], worst


def _has_partner(box, cls, other_box, other_cls, px):
    """For every (box, cls): is there a same-class box in the other set with every coordinate within px?"""
    box, other_box = np.asarray(box, np.float64).reshape(-1, 4), np.asarray(other_box, np.float64).reshape(-1, 4)
    cls, other_cls = np.asarray(cls), np.asarray(other_cls)
    if len(box) == 0:
        return np.zeros(0, bool)
    if len(other_box) == 0:
        return np.zeros(len(box), bool)
    d = np.abs(box[:, None, :] - other_box[None, :, :]).max(axis=2)
    d[cls[:, None] != other_cls[None, :]] = np.inf
    return d.min(axis=1) <= px


def selection_sets(got_box, got_cls, runs, px=1.0):
    """The set-valued parity statement for an ill-conditioned selection (greedy NMS): `runs` = [(boxes, classes)] are the
    oracle's own detections on its logits, unperturbed (first) and perturbed by noise of the device's error size.
    core  = boxes of run 0 that every run keeps (their fate does not depend on the rounding noise),
    union = boxes that some run keeps.
    -> (core boxes the device lacks, device boxes outside the union, |core|, |union| summed over the runs)."""
    b0, k0 = runs[0]
    in_all = np.ones(len(b0), bool)
    for b, k in runs[1:]:
        in_all &= _has_partner(b0, k0, b, k, px)
    core_b, core_k = np.asarray(b0).reshape(-1, 4)[in_all], np.asarray(k0)[in_all]
    ub = np.concatenate([np.asarray(b, np.float64).reshape(-1, 4) for b, _ in runs])
    uk = np.concatenate([np.asarray(k) for _, k in runs])
    core_missing = int((~_has_partner(core_b, core_k, got_box, got_cls, px)).sum())
    outside = int((~_has_partner(got_box, got_cls, ub, uk, px)).sum())
    return core_missing, outside, int(in_all.sum()), len(ub)


def spread_params(seed=0):
    """The seeded random YOLOv8n-topology parameter vector with the Detect head's final class convolutions rescaled so
    that confidences spread over (0, 1) instead of sitting within 1e-3 of each other (which is what plain random
    initialisation gives: every anchor passes the 0.25 filter and the NMS order is decided by rounding noise).
    Test input only: weights x 30, biases - 8 on the three 80 -> 80 1x1 convolutions (about 200 of the 5040 anchors
    then pass the filter, with a median confidence gap of 5e-4 between neighbours in the sorted list)."""
    from oracle import yolo_ref as R
    p = R.random_params(seed).copy()
    pos = 0
    for cin, cout, k, _, bn in R.conv_specs():
        nw = cout * cin * k * k
        if not bn and cout == R.NC:
            p[pos:pos + nw] *= 30.0
            p[pos + nw:pos + nw + cout] -= 8.0
        pos += nw + (4 * cout if bn else cout)
    assert pos == p.size
    return p


class LaneBatch:
    """One av_lane_detect batch on cuda:0: the workspace (zero-filled by av_lane_workspace_init), the per-frame
    state / poly / pts / info / conf tensors and, by default, the configuration lane_detector.py uses (HoughLinesP 50, 50,
    150; smoothing 0.7).  `bgr`: frames as a list of arrays, a u8 device tensor [S][h][w][3], or None (run() is then given one,
    or the batch only runs the Hough / fit stages on lists written by load_points / load_segments, or the pixel stages on gray
    images written by load_gray)."""

    def __init__(self, S, h, w, MS, bgr=None, threshold=50, min_line_length=50, max_line_gap=150, smoothing=0.7):
        import torch
        from multimodal_autonomous_driving_perception_and_planning_amd import _native as nat
        self.S, self.h, self.w, self.MS = S, h, w, MS
        self.nat, self.L, self.ctx, self.sh = nat, nat.lib(), nat.default_context(0), nat.stream_handle()
        dev = torch.device("cuda", 0)
        self.bgr = torch.as_tensor(np.stack(bgr)).to(dev) if isinstance(bgr, (list, tuple)) else bgr
        self.ws = torch.empty(int(self.L.av_lane_workspace_bytes(S, h, w, MS)), dtype=torch.uint8, device=dev)
        nat.check(self.L.av_lane_workspace_init(self.ctx.handle, self.sh, S, h, w, MS, nat.ptr(self.ws)))
        self.state = torch.zeros(S, 8, dtype=torch.float64, device=dev)
        self.poly = torch.zeros(S, 2, 3, dtype=torch.float64, device=dev)
        self.pts = torch.zeros(S, 2, 50, 2, dtype=torch.int32, device=dev)
        self.info = torch.zeros(S, 8, dtype=torch.int32, device=dev)
        self.conf = torch.zeros(S, 2, dtype=torch.float64, device=dev)
        self.cfg = nat.LaneCfg(threshold, min_line_length, max_line_gap, MS, smoothing)

    def run(self, stages, bgr=None, roi_rows=None):
        """av_lane_detect on the whole batch, then a device synchronize.  roi_rows: None (the default trapezoid) or the caller's ROI,
        int32 [h][2] = inclusive [xl, xr] per row (xl > xr: an empty row), shared by the frames of the batch."""
        import ctypes as C
        import torch
        nat = self.nat
        if bgr is None and self.bgr is None and (stages & (16 | 64)):
            self.bgr = torch.zeros(256, dtype=torch.uint8, device=self.ws.device)      # never read: no BGR stage runs
        roi = None
        if roi_rows is not None:
            roi_rows = np.ascontiguousarray(roi_rows, np.int32)
            assert roi_rows.shape == (self.h, 2)
            roi = torch.as_tensor(roi_rows).to(self.ws.device)
        nat.check(self.L.av_lane_detect(self.ctx.handle, self.sh, C.byref(self.cfg), self.S, self.h, self.w,
                                        nat.ptr(self.bgr if bgr is None else bgr), nat.ptr(roi) if roi is not None else None,
                                        nat.ptr(self.ws), nat.ptr(self.state),
                                        nat.ptr(self.poly), nat.ptr(self.pts), nat.ptr(self.info), nat.ptr(self.conf), stages))
        torch.cuda.synchronize()

    def span(self, what):
        """(byte offset, byte count) of workspace view `what` (av_lane_workspace_view)."""
        import ctypes as C
        off, nb = C.c_size_t(), C.c_size_t()
        self.nat.check(self.L.av_lane_workspace_view(what, self.S, self.h, self.w, self.MS, C.byref(off), C.byref(nb)))
        return off.value, nb.value

    def view(self, what, dtype, shape):
        """Workspace view `what`, copied to the host."""
        off, nb = self.span(what)
        return self.ws[off:off + nb].cpu().numpy().view(dtype).reshape(shape)

    def _put(self, what, offset, arr):
        """Bytes of `arr` into workspace view `what` at byte `offset`."""
        import torch
        off, nb = self.span(what)
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert offset + raw.size <= nb
        self.ws[off + offset:off + offset + raw.size].copy_(torch.as_tensor(raw))

    def load_gray(self, s, image, lo, hi):
        """Frame s's input of a given-gray call (stage bit 64): the u8 image (view 0) and its Canny thresholds (view 4: lo, hi as
        doubles)."""
        image = np.array(image, np.uint8)               # a writable copy: torch.as_tensor refuses read-only arrays
        assert image.shape == (self.h, self.w)
        self._put(0, s * self.h * self.w, image)
        self._put(4, 32 * s, np.array([lo, hi], np.float64))

    def points(self, s):
        """Frame s's point list as the pixel stages left it (views 9 / 10): uint32 x | y << 16."""
        n = int(self.view(10, np.int32, (self.S,))[s])
        assert 0 <= n <= self.h * self.w
        return self.view(9, np.uint32, (self.S, self.h * self.w))[s, :n].copy()

    def load_points(self, s, edge_map):
        """Frame s's Hough input as the pixel stages would leave it for `edge_map` (u8 [h][w], non-zero = edge): the row-major
        point list x | y << 16 (view 9), its length (view 10) and the masked byte map (view 3: what the generic kernel reads
        when the frame shape has no bit-map path).  The Hough stage consumes the list: reload it before every run."""
        assert edge_map.shape == (self.h, self.w)
        ys, xs = np.nonzero(edge_map)
        pts = xs.astype(np.uint32) | (ys.astype(np.uint32) << 16)
        if len(pts):
            self._put(9, 4 * s * self.h * self.w, pts)
        self._put(10, 4 * s, np.array([len(pts)], np.int32))
        self._put(3, s * self.h * self.w, np.where(edge_map != 0, 255, 0).astype(np.uint8))
        return len(pts)

    def load_segments(self, s, segs):
        """Frame s's segment list (view 5, rows x1 y1 x2 y2) and its length (view 6): input of a fit-only call (stage bits 16 | 32)."""
        segs = np.asarray(segs, np.int32).reshape(-1, 4)
        assert len(segs) <= self.MS
        buf = np.zeros((self.MS, 4), np.int32)
        buf[:len(segs)] = segs
        self._put(5, 16 * s * self.MS, buf)
        self._put(6, 4 * s, np.array([len(segs)], np.int32))
