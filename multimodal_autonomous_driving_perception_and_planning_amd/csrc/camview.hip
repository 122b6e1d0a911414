// The demo's annotated view composed on the device: what demo.py:122-150 builds per frame with six class calls --
// detector.draw_detections, lane_detector.draw_lanes, tracker.draw_tracks, overlay.draw_info_panel, draw_detection_summary,
// create_side_by_side (and, off in the demo, draw_lane_offset_indicator) -- from the tables a CameraLoop step leaves in HBM.
//
//   av_camview_build   one workgroup per camera writes the camera view's av_prim list (compacted, in the classes' order) and the
//                      lane polygon's vertex list; av_raster_draw / av_raster_draw_to paints it
//   av_view_compose    camera picture | BEV panel at the taller one's height, with the two labels, one launch for S cameras
//   av_bgr_to_i420     the combined pictures as planar 4:2:0 for an uncompressed video file (loaders.Y4MWriter)
//   av_format_fixed    the number text of the overlays (fmtnum.h) for the host
#include "common.h"
#include "fmtnum.h"
#include "raster_dev.h"

namespace {

using namespace rasterdev;

constexpr int CV_ITEMS = 1024;         // detections / track rows per camera the builder indexes in LDS
constexpr int CV_LINE = 48;            // longest text line: "Pos: (" + 14 + ", " + 14 + ")" = 37; name 23 + ' ' + 14 = 38
constexpr int CV_NUM = fmtnum::MAX_FIXED - 2;      // 14: "-1000000000.00"
constexpr int CV_INT = fmtnum::MAX_INT;            // 11
constexpr int CV_LANE_PTS = 50;
constexpr unsigned WHITE = 0xFFFFFFu;

__host__ __device__ inline int det_name_cap(int max_name) { return max_name > 7 ? max_name : 7; }          // "unknown"
__host__ __device__ inline int trk_name_cap(int max_name) { return max_name > CV_INT ? max_name : CV_INT; }   // or the class id
__host__ __device__ inline int det_slots(int max_name) { return 4 + 1 + det_name_cap(max_name) + 1 + CV_NUM; }
__host__ __device__ inline int trk_slots(int max_name, int L) { return 4 + 3 + CV_INT + 1 + trk_name_cap(max_name) + (L - 1); }
__host__ __device__ inline int sum_slots(int max_name) { return 2 + det_name_cap(max_name) + 2 + CV_INT; }
constexpr int LANE_SLOTS = 1 + 2 * (CV_LANE_PTS - 1);
constexpr int INFO_SLOTS = 1 + (7 + CV_INT) + (5 + CV_NUM) + (7 + CV_NUM + 5) + (9 + CV_NUM + 4) + (7 + CV_NUM + 5) + (6 + CV_NUM + 2 + CV_NUM + 1);
constexpr int GAUGE_SLOTS = 1 + 4 + 1 + 1 + (8 + CV_NUM + 2);

// writes primitives at out[0 ..), or only counts them (out == nullptr); never past `limit`
struct Emit {
    av_prim* out;
    int limit, n;
    __device__ void put(const av_prim& q) {
        if (out && n < limit) out[n] = q;
        ++n;
    }
    __device__ void seg(int x0, int y0, int x1, int y1, int th, unsigned col) { put(mk(AV_PRIM_SEG, x0, y0, x1, y1, th > 1 ? th : 1, col)); }
    // PrimList.rectangle with thickness >= 0: the four sides, clockwise from the top
    __device__ void outline(int x0, int y0, int x1, int y1, int th, unsigned col) {
        seg(x0, y0, x1, y0, th, col), seg(x1, y0, x1, y1, th, col), seg(x1, y1, x0, y1, th, col), seg(x0, y1, x0, y0, th, col);
    }
    // PrimList.put_text at font scales below 0.55: org is the text's bottom-left corner; blanks advance, nothing is drawn for them
    __device__ void text(const char* s, int len, int x, int y_base, unsigned col) {
        for (int k = 0; k < len; ++k) {
            const int code = (unsigned char)s[k];
            if (code > 32 && code <= 126) put(mk(AV_PRIM_GLYPH, x + 6 * k, y_base - 7, 1, 0, code, col));
        }
    }
};

// a text line put together from pieces; CV_LINE bounds every line the builder writes (the pieces' own caps add up to less)
struct Line {
    char s[CV_LINE];
    int n = 0;
    __device__ void lit(const char* t) {
        for (; *t && n < CV_LINE; ++t) s[n++] = *t;
    }
    __device__ void chars(const char* t, int len) {
        for (int k = 0; k < len && n < CV_LINE; ++k) s[n++] = t[k];
    }
    __device__ void fixed(double v, int d) {
        const int k = fmtnum::fmt_fixed(v, d, s + n, CV_LINE - n);
        if (k > 0) n += k;
    }
    __device__ void integer(int v) {
        const int k = fmtnum::fmt_int(v, s + n, CV_LINE - n);
        if (k > 0) n += k;
    }
};

struct NameTable {
    const char* names;              // char [n][AV_NAME_BYTES]
    const int32_t* lens;            // int32 [n]; negative = no such id
    int n, max_name;
    __device__ int get(int id, const char*& s) const {
        if (id < 0 || id >= n || lens[id] < 0) return -1;
        s = names + (size_t)id * AV_NAME_BYTES;
        return min(min(lens[id], max_name), AV_NAME_BYTES - 1);
    }
};

// one layer of the list: `count` items, item i writes item(i, e); the items' primitives follow each other in item order
template <class F>
__device__ void layer(int count, av_prim* out, int cap, int& base, int* cnt, F item) {
    const int tid = threadIdx.x;
    for (int i = tid; i < count; i += 256) {
        Emit e{nullptr, 0, 0};
        item(i, e);
        cnt[i] = e.n;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int i = 0; i < count; ++i) {
            const int v = cnt[i];
            cnt[i] = acc, acc += v;
        }
        cnt[count] = acc;
    }
    __syncthreads();
    for (int i = tid; i < count; i += 256) {
        const int at = base + cnt[i];
        Emit e{out + at, at < cap ? cap - at : 0, 0};
        item(i, e);
    }
    base += cnt[count];
    __syncthreads();
}

__global__ void __launch_bounds__(256) camview_build_kernel(av_camview_args a, av_prim* __restrict__ prims, int prim_cap,
                                                            int32_t* __restrict__ n_prims, int32_t* __restrict__ verts, int vert_cap,
                                                            size_t trk_bytes) {
    __shared__ int cnt[CV_ITEMS + 2];          // the summary has one item more than there are detections, plus the total
    __shared__ short canon[CV_ITEMS], rank[CV_ITEMS], same[CV_ITEMS];
    __shared__ int s_distinct;
    const int s = blockIdx.x, tid = threadIdx.x;
    av_prim* out = prims + (size_t)s * prim_cap;
    int base = 0;
    const size_t sf = (size_t)s * a.n_frames + a.frame;
    const NameTable dnames{a.det_names, a.det_name_len, a.n_det_names, a.max_name};
    const NameTable tnames{a.trk_names, a.trk_name_len, a.n_trk_names, a.max_name};
    const int nd = (a.flags & (AV_VIEW_DETECTIONS | AV_VIEW_SUMMARY)) ? max(0, min(a.det_n[s], a.max_det)) : 0;
    const int32_t* dcls = a.det_cls + (size_t)s * a.max_det;
    const int32_t* info = a.lane_info ? a.lane_info + (size_t)s * 8 : nullptr;
    const int32_t* lpts = a.lane_pts ? a.lane_pts + (size_t)s * 2 * CV_LANE_PTS * 2 : nullptr;
    const bool left = info && info[0] != 0, right = info && info[1] != 0;

    // ---- 1. detections (ObjectDetector.draw_detections): box outline, filled label box, "name 0.87" -------------------------
    if (a.flags & AV_VIEW_DETECTIONS) {
        const float* box = a.det_box + (size_t)s * a.max_det * 4;
        const float* conf = a.det_conf + (size_t)s * a.max_det;
        layer(nd, out, prim_cap, base, cnt, [&](int i, Emit& e) {
            const int x1 = (int)box[4 * i], y1 = (int)box[4 * i + 1], x2 = (int)box[4 * i + 2], y2 = (int)box[4 * i + 3], c = dcls[i];
            unsigned col = WHITE;
            if (c >= 0 && c < a.n_det_colors) col = a.det_colors[3 * c] | (a.det_colors[3 * c + 1] << 8) | (a.det_colors[3 * c + 2] << 16);
            e.outline(x1, y1, x2, y2, 2, col);
            Line t;
            const char* nm = nullptr;
            const int nl = dnames.get(c, nm);
            if (nl >= 0) t.chars(nm, nl);
            else t.lit("unknown");
            t.lit(" ");
            t.fixed((double)conf[i], 2);
            e.put(mk(AV_PRIM_RECT, x1, y1 - 19, x1 + 6 * t.n + 5, y1, 0, col));
            e.text(t.s, t.n, x1 + 2, y1 - 5, 0u);
        });
    }
    // ---- 2. lanes (LaneDetector.draw_lanes): the blended lane area, then the two fitted lines -------------------------------
    if ((a.flags & AV_VIEW_LANES) && lpts) {
        const int32_t* lp = lpts;
        const int32_t* rp = lpts + CV_LANE_PTS * 2;
        if (left && right) {
            int32_t* v = verts + (size_t)s * vert_cap * 2;
            for (int k = tid; k < 2 * CV_LANE_PTS; k += 256) {
                const int32_t* p = k < CV_LANE_PTS ? lp + 2 * k : rp + 2 * (2 * CV_LANE_PTS - 1 - k);
                v[2 * k] = p[0], v[2 * k + 1] = p[1];
            }
        }
        layer(LANE_SLOTS, out, prim_cap, base, cnt, [&](int i, Emit& e) {
            if (i == 0) {
                if (!(left && right)) return;
                int xlo = lp[0], xhi = lp[0], ylo = lp[1], yhi = lp[1];
                for (int k = 0; k < 2 * CV_LANE_PTS; ++k) {
                    const int32_t* p = k < CV_LANE_PTS ? lp + 2 * k : rp + 2 * (k - CV_LANE_PTS);
                    xlo = min(xlo, p[0]), xhi = max(xhi, p[0]), ylo = min(ylo, p[1]), yhi = max(yhi, p[1]);
                }
                av_prim q = mk(AV_PRIM_POLY_BLEND, 0, 2 * CV_LANE_PTS, 0, 0, 0, 0x64FF00u);            // (0, 255, 100)
                q.x2 = xlo, q.y2 = ylo, q.x3 = xhi, q.y3 = yhi;
                e.put(q);
                return;
            }
            const int side = (i - 1) / (CV_LANE_PTS - 1), k = (i - 1) % (CV_LANE_PTS - 1);
            if (!(side ? right : left)) return;
            const int32_t* p = (side ? rp : lp) + 2 * k;
            e.seg(p[0], p[1], p[2], p[3], 3, side ? 0xFF0000u : 0x0000FFu);
        });
    }
    // ---- 3. tracks (MultiObjectTracker.draw_tracks): confirmed rows in table order: box, "ID:n name", trail ----------------------
    if (a.flags & AV_VIEW_TRACKS) {
        const av_track_row* rows = a.snap + sf * a.tcap;
        const int nrows = max(0, min(a.snap_n[sf], a.tcap)), L = a.trajectory_length;
        const double* hist = reinterpret_cast<const double*>((const uint8_t*)a.tracker_state + (size_t)s * trk_bytes + 64 + (size_t)a.tcap * 64);
        layer(nrows, out, prim_cap, base, cnt, [&](int i, Emit& e) {
            const av_track_row r = rows[i];
            if (!(r.flags & 1)) return;
            const unsigned palette[8] = {0x0000FFu, 0x00FF00u, 0xFF0000u, 0x00FFFFu, 0xFF00FFu, 0xFFFF00u, 0xFF0080u, 0x0080FFu};
            const unsigned col = palette[((r.id % 8) + 8) % 8];
            e.outline(r.x1, r.y1, r.x2, r.y2, 2, col);
            Line t;
            t.lit("ID:");
            t.integer(r.id);
            t.lit(" ");
            const char* nm = nullptr;
            const int nl = tnames.get(r.cls, nm);
            if (nl >= 0) t.chars(nm, nl);
            else t.integer(r.cls);
            e.text(t.s, t.n, r.x1, r.y1 - 10, col);
            const int len = min(r.hist_len, L), first = r.hist_len - len;
            if (r.slot < 0 || r.slot >= a.tcap) return;
            for (int j = 1; j < len; ++j) {
                const double* p = hist + ((size_t)r.slot * L + (size_t)((first + j - 1) % L)) * 4;
                const double* q = hist + ((size_t)r.slot * L + (size_t)((first + j) % L)) * 4;
                e.seg((int)p[0], (int)p[1], (int)q[0], (int)q[1], 3 * j / len, col);
            }
        });
    }
    // ---- 4. info panel (OverlayRenderer.draw_info_panel) -------------------------------------------------------------------------
    if (a.flags & AV_VIEW_INFO) {
        const double* v = a.vstate ? a.vstate + sf * AV_VSTATE_DOUBLES : nullptr;
        const int32_t* hdr = reinterpret_cast<const int32_t*>((const uint8_t*)a.tracker_state + (size_t)s * trk_bytes);
        layer(v ? 7 : 3, out, prim_cap, base, cnt, [&](int i, Emit& e) {
            if (i == 0) {
                e.put(mk(AV_PRIM_BLEND_RECT, 10, 10, 250, 150, 0, 0u));
                return;
            }
            Line t;
            switch (i) {
                case 1: t.lit("Frame: "), t.integer(hdr[2] - 1); break;
                case 2: t.lit("FPS: "), t.fixed(a.fps, 1); break;
                case 3: t.lit("Speed: "), t.fixed(v[5] * 3.6, 1), t.lit(" km/h"); break;
                case 4: t.lit("Heading: "), t.fixed(v[4] * (180.0 / 3.141592653589793), 1), t.lit(" deg"); break;
                case 5: t.lit("Accel: "), t.fixed(v[6], 2), t.lit(" m/s2"); break;
                default: t.lit("Pos: ("), t.fixed(v[0], 1), t.lit(", "), t.fixed(v[1], 1), t.lit(")"); break;
            }
            e.text(t.s, t.n, 20, 30 + 20 * (i - 1), WHITE);
        });
    }
    // ---- 5. detection summary, top right: a count per class name in order of first appearance ------------------------------------
    if (a.flags & AV_VIEW_SUMMARY) {
        // every id outside the name table is the one name "unknown"
        for (int i = tid; i < nd; i += 256) {
            const char* nm;
            canon[i] = (short)(dnames.get(dcls[i], nm) >= 0 ? dcls[i] : -1);
        }
        __syncthreads();
        for (int i = tid; i < nd; i += 256) {
            int before = 0, all = 0;
            for (int j = 0; j < nd; ++j) {
                const int eq = canon[j] == canon[i];
                all += eq, before += eq && j < i;
            }
            same[i] = (short)all, rank[i] = (short)(before == 0);
        }
        __syncthreads();
        if (tid == 0) {
            int acc = 0;
            for (int i = 0; i < nd; ++i) {
                const int f = rank[i];
                rank[i] = (short)(f ? acc : -1), acc += f;
            }
            s_distinct = acc;
        }
        __syncthreads();
        const int x0 = a.w - 150, y0 = 10, distinct = s_distinct;
        layer(nd + 1, out, prim_cap, base, cnt, [&](int i, Emit& e) {
            if (i == 0) {
                e.put(mk(AV_PRIM_BLEND_RECT, x0, y0, x0 + 140, y0 + 20 + distinct * 18, 0, 0u));
                e.text("Detections:", 11, x0 + 5, y0 + 15, WHITE);
                return;
            }
            const int d = i - 1;
            if (rank[d] < 0) return;
            Line t;
            t.lit("  ");
            const char* nm = nullptr;
            const int nl = dnames.get(dcls[d], nm);
            if (nl >= 0) t.chars(nm, nl);
            else t.lit("unknown");
            t.lit(": ");
            t.integer(same[d]);
            e.text(t.s, t.n, x0 + 5, y0 + 35 + 18 * rank[d], 0xC8C8C8u);
        });
    }
    // ---- 6. lane-offset gauge (OverlayRenderer.draw_lane_offset_indicator, fed get_lane_center_offset) ---------------------------
    if (a.flags & AV_VIEW_GAUGE) {
        layer(1, out, prim_cap, base, cnt, [&](int, Emit& e) {
            const int iw = 200, ih = 30, x0 = (a.w - iw) >> 1, y0 = a.h - 50, cx = x0 + iw / 2;
            e.put(mk(AV_PRIM_RECT, x0, y0, x0 + iw, y0 + ih, 0, 0x323232u));
            e.outline(x0, y0, x0 + iw, y0 + ih, 1, 0x646464u);
            e.seg(cx, y0, cx, y0 + ih, 1, WHITE);
            if (!(left && right && lpts)) return;
            const int lx = lpts[2 * (CV_LANE_PTS - 1)], rx = lpts[2 * CV_LANE_PTS + 2 * (CV_LANE_PTS - 1)];
            const double off = (double)a.w / 2.0 - (double)(lx + rx) / 2.0, mag = fabs(off);
            const int o = (int)(off < -100.0 ? -100.0 : off > 100.0 ? 100.0 : off);
            e.put(mk(AV_PRIM_DISC, cx + o, y0 + ih / 2, 0, 0, 8, mag < 20.0 ? 0x00FF00u : mag < 50.0 ? 0xFFFF00u : 0xFF0000u));
            Line t;
            t.lit("Offset: "), t.fixed(off, 0), t.lit("px");
            e.text(t.s, t.n, x0 + 5, y0 - 5, WHITE);
        });
    }
    if (tid == 0) n_prims[s] = min(base, prim_cap);
}

// ---- camera picture | BEV panel, both at the taller one's height, and the two labels (create_side_by_side) -----------------------
struct ViewLabels {
    char s[2][AV_VIEW_LABEL_BYTES];
    int len[2];
};

__device__ __forceinline__ bool label_covers(const ViewLabels& lb, int which, int x0, int x, int y) {
    // put_text(label, (x0, 25), 0.6, ...): the doubled font, top row 25 - 14, 12 columns per character
    const int gx = x - x0, gy = y - 11;
    if (gx < 0 || gy < 0 || gy >= 14 || gx >= 12 * lb.len[which]) return false;
    const int code = (unsigned char)lb.s[which][gx / 12];
    return code > 32 && glyph_bit(code, gx % 12, gy, 2);
}

__global__ void __launch_bounds__(256) view_compose_kernel(const uint8_t* __restrict__ cam, int h1, int w1, const uint8_t* __restrict__ bev,
                                                           int h2, int w2, uint8_t* __restrict__ out, int th, int nw1, int nw2, ViewLabels lb) {
    const int i = blockIdx.x * 256 + threadIdx.x, tw = nw1 + nw2, s = blockIdx.y;
    if (i >= th * tw) return;
    const int y = i / tw, x = i - y * tw;
    uint8_t* o = out + (((size_t)s * th + y) * tw + x) * 3;
    if (label_covers(lb, 0, 10, x, y) || label_covers(lb, 1, nw1 + 10, x, y)) {
        o[0] = o[1] = o[2] = 255;
        return;
    }
    const bool second = x >= nw1;
    const uint8_t* src = second ? bev : cam;
    if (!src) return;                                     // that half was painted in place (av_raster_draw_to)
    const int sh = second ? h2 : h1, sw = second ? w2 : w1, dw = second ? nw2 : nw1, dx = second ? x - nw1 : x;
    src += (size_t)s * sh * sw * 3;
    if (sh == th) {
        const uint8_t* p = src + ((size_t)y * sw + dx) * 3;
        o[0] = p[0], o[1] = p[1], o[2] = p[2];
    } else {
        const ResizeTap t = resize_tap(sh, sw, th, dw, dx, y);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = resize_channel(src, sw, t, k);
    }
}

// ---- interleaved BGR -> planar I420, BT.601 limited range in OpenCV's published 20-bit constants (cvtColor COLOR_BGR2YUV_I420:
// CRY 269484, CGY 528482, CBY 102760, CRU -155188, CGU -305135, CBU = CRV 460324, CGV -385875, CBV -74448), parity unpinned.
// A thread makes one 2x2 block: four luma samples and the chroma pair of the block's rounded mean colour.
__global__ void __launch_bounds__(256) bgr_to_i420_kernel(const uint8_t* __restrict__ bgr, int n, int h, int w, uint8_t* __restrict__ yuv) {
    const int i = blockIdx.x * 256 + threadIdx.x, w2 = w >> 1, h2 = h >> 1;
    if (i >= n * h2 * w2) return;
    const int f = i / (h2 * w2), r = i - f * h2 * w2, by = r / w2, bx = r - by * w2;
    const uint8_t* src = bgr + (size_t)f * h * w * 3;
    uint8_t* Y = yuv + (size_t)f * ((size_t)h * w * 3 / 2);
    uint8_t* U = Y + (size_t)h * w;
    uint8_t* V = U + (size_t)h2 * w2;
    int sb = 0, sg = 0, sr = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = 2 * by + (k >> 1), x = 2 * bx + (k & 1);
        const uint8_t* p = src + ((size_t)y * w + x) * 3;
        const int b = p[0], g = p[1], rr = p[2];
        sb += b, sg += g, sr += rr;
        Y[(size_t)y * w + x] = (uint8_t)min(max((269484 * rr + 528482 * g + 102760 * b + (16 << 20) + (1 << 19)) >> 20, 0), 255);
    }
    const int b = (sb + 2) >> 2, g = (sg + 2) >> 2, rr = (sr + 2) >> 2;
    U[(size_t)by * w2 + bx] = (uint8_t)min(max((-155188 * rr - 305135 * g + 460324 * b + (128 << 20) + (1 << 19)) >> 20, 0), 255);
    V[(size_t)by * w2 + bx] = (uint8_t)min(max((460324 * rr - 385875 * g - 74448 * b + (128 << 20) + (1 << 19)) >> 20, 0), 255);
}

}  // namespace

extern "C" {

int av_format_fixed(double v, int decimals, char* out, int cap) {
    if (!out || cap < 0 || decimals < 0 || decimals > 2) return AV_EINVAL;
    return fmtnum::fmt_fixed(v, decimals, out, cap);
}

int av_camview_prim_cap(int max_det, int tcap, int trajectory_length, int max_name) {
    if (max_det < 0 || tcap < 0 || trajectory_length < 1 || max_name < 0 || max_name >= AV_NAME_BYTES || max_det > CV_ITEMS || tcap > CV_ITEMS)
        return 0;
    return max_det * det_slots(max_name) + LANE_SLOTS + tcap * trk_slots(max_name, trajectory_length) + INFO_SLOTS + 1 + 11 +
           max_det * sum_slots(max_name) + GAUGE_SLOTS;
}

int av_camview_build(av_ctx* ctx, av_stream_t stream, const av_camview_args* a, av_prim* prims, int prim_cap, int32_t* n_prims,
                     int32_t* verts, int vert_cap) {
    AV_REQUIRE(ctx && a && prims && n_prims, AV_EINVAL, "av_camview_build: null argument");
    AV_REQUIRE(a->n_streams > 0 && a->h > 0 && a->w > 0 && a->h < 8192 && a->w < 8192 && a->n_frames > 0 && a->frame >= 0 &&
                   a->frame < a->n_frames, AV_EINVAL, "av_camview_build: bad dimensions");
    AV_REQUIRE((a->flags & ~AV_VIEW_ALL) == 0, AV_EINVAL, "av_camview_build: unknown layer bits 0x%x", a->flags);
    AV_REQUIRE(a->max_name >= 0 && a->max_name < AV_NAME_BYTES, AV_EINVAL, "av_camview_build: max_name is 0 .. %d", AV_NAME_BYTES - 1);
    AV_REQUIRE(a->max_det >= 0 && a->max_det <= CV_ITEMS && a->tcap >= 0 && a->tcap <= CV_ITEMS && a->trajectory_length >= 1, AV_EINVAL,
               "av_camview_build: max_det and tcap are 0 .. %d, trajectory_length >= 1", CV_ITEMS);
    if (a->flags & (AV_VIEW_DETECTIONS | AV_VIEW_SUMMARY))
        AV_REQUIRE(a->det_n && a->det_cls && a->max_det > 0 && (a->n_det_names == 0 || (a->det_names && a->det_name_len)) && a->n_det_names >= 0 &&
                       a->n_det_names < 32768, AV_EINVAL, "av_camview_build: the detection layers need det_n, det_cls and the name table");
    if (a->flags & AV_VIEW_DETECTIONS)
        AV_REQUIRE(a->det_box && a->det_conf && a->n_det_colors >= 0 && (a->n_det_colors == 0 || a->det_colors), AV_EINVAL,
                   "av_camview_build: the detection layer needs det_box, det_conf and the colour table");
    if (a->flags & (AV_VIEW_LANES | AV_VIEW_GAUGE))
        AV_REQUIRE(a->lane_pts && a->lane_info, AV_EINVAL, "av_camview_build: the lane layers need lane_pts and lane_info");
    if (a->flags & AV_VIEW_LANES)
        AV_REQUIRE(verts && vert_cap >= 2 * CV_LANE_PTS, AV_EINVAL, "av_camview_build: the lane area needs %d vertices per camera", 2 * CV_LANE_PTS);
    if (a->flags & (AV_VIEW_TRACKS | AV_VIEW_INFO))
        AV_REQUIRE(a->tracker_state && a->tcap > 0, AV_EINVAL, "av_camview_build: the track and info layers need the tracker's state");
    if (a->flags & AV_VIEW_TRACKS)
        AV_REQUIRE(a->snap && a->snap_n && a->n_trk_names >= 0 && (a->n_trk_names == 0 || (a->trk_names && a->trk_name_len)), AV_EINVAL,
                   "av_camview_build: the track layer needs snap, snap_n and the name table");
    const int need = av_camview_prim_cap(a->max_det, a->tcap, a->trajectory_length, a->max_name);
    AV_REQUIRE(need > 0 && need <= 65535, AV_EINVAL, "av_camview_build: the list may need %d primitives, the rasteriser takes 65535", need);
    AV_REQUIRE(prim_cap >= need && prim_cap <= 65535, AV_EINVAL, "av_camview_build: prim_cap %d, need %d (<= 65535)", prim_cap, need);
    hipLaunchKernelGGL(camview_build_kernel, dim3(a->n_streams), dim3(256), 0, as_stream(stream), *a, prims, prim_cap, n_prims, verts, vert_cap,
                       a->tcap > 0 ? av_tracker_state_bytes(a->tcap, a->trajectory_length) : (size_t)0);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_view_compose_size(int h1, int w1, int h2, int w2, int* th, int* nw1, int* nw2) {
    AV_REQUIRE(th && nw1 && nw2, AV_EINVAL, "av_view_compose_size: null argument");
    AV_REQUIRE(h1 > 0 && w1 > 0 && h2 > 0 && w2 > 0 && h1 < 8192 && w1 < 8192 && h2 < 8192 && w2 < 8192, AV_EINVAL,
               "av_view_compose_size: bad picture sizes %dx%d, %dx%d", w1, h1, w2, h2);
    // overlays.py:88-90: th = max(h1, h2); nw = w if h == th else int(w * (th / h))
    const int t = h1 > h2 ? h1 : h2;
    *th = t;
    *nw1 = h1 == t ? w1 : (int)((double)w1 * ((double)t / (double)h1));
    *nw2 = h2 == t ? w2 : (int)((double)w2 * ((double)t / (double)h2));
    return AV_OK;
}

int av_view_compose(av_ctx* ctx, av_stream_t stream, int n_images, const uint8_t* cam, int h1, int w1, const uint8_t* bev, int h2, int w2,
                    uint8_t* out, const char* label1, const char* label2) {
    AV_REQUIRE(ctx && out && label1 && label2 && (cam || bev), AV_EINVAL, "av_view_compose: null argument");
    int th, nw1, nw2;
    if (const int rc = av_view_compose_size(h1, w1, h2, w2, &th, &nw1, &nw2)) return rc;
    AV_REQUIRE(n_images > 0 && nw1 > 0 && nw2 > 0 && (long long)th * (nw1 + nw2) < (1LL << 30), AV_EINVAL, "av_view_compose: bad geometry");
    AV_REQUIRE(cam || h1 == th, AV_EINVAL, "av_view_compose: a camera half left in place has to keep its size");
    AV_REQUIRE(bev || h2 == th, AV_EINVAL, "av_view_compose: a panel half left in place has to keep its size");
    ViewLabels lb{};
    const char* ls[2] = {label1, label2};
    for (int k = 0; k < 2; ++k) {
        int n = 0;
        while (ls[k][n]) {
            AV_REQUIRE(n < AV_VIEW_LABEL_BYTES - 1, AV_EINVAL, "av_view_compose: a label has at most %d characters", AV_VIEW_LABEL_BYTES - 1);
            lb.s[k][n] = ls[k][n], ++n;
        }
        lb.len[k] = n;
    }
    const int npx = th * (nw1 + nw2);
    hipLaunchKernelGGL(view_compose_kernel, dim3((npx + 255) / 256, n_images), dim3(256), 0, as_stream(stream), cam, h1, w1, bev, h2, w2, out, th,
                       nw1, nw2, lb);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_bgr_to_i420(av_ctx* ctx, av_stream_t stream, int n_frames, int h, int w, const uint8_t* bgr, uint8_t* yuv) {
    AV_REQUIRE(ctx && bgr && yuv, AV_EINVAL, "av_bgr_to_i420: null argument");
    AV_REQUIRE(n_frames > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0, AV_EINVAL, "av_bgr_to_i420: 4:2:0 frames need even sizes, got %dx%d", w, h);
    const long long n = (long long)n_frames * (h / 2) * (w / 2);
    AV_REQUIRE(n < (1LL << 31), AV_EINVAL, "av_bgr_to_i420: too many pixels in one call");
    hipLaunchKernelGGL(bgr_to_i420_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), bgr, n_frames, h, w, yuv);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // extern "C"
