// The tag log: what AutoTagger keeps per frame (auto_tagger.py:112-310: all_tags, tag_counts, search_by_tag(s), get_high_risk_frames,
// get_event_segments, get_tag_statistics), resident on the device for S streams.
//
// A logged frame is one 64-bit mask over the fixed vocabulary of include/avhot.h (AV_TAG_*: 49 tags in the reference's Enum definition
// order, three presence flags in bits 61..63) plus the frame's speed.  av_tags_pack joins the three taggers' rows of S x W frames into
// masks (the get_tags_list of scene_classifier.py:66, maneuver_detector.py:71, interaction_detector.py:95);
// av_taglog_append moves them into the log behind log_n[s], which lives on the device; the queries are kernels over the masks.
//
// Mapping.  Pack: one wave per frame, lane = list entry (interaction row, detection) in rounds of 64, OR across the wave.  Append: one
// workgroup per stream (every thread reads log_n[s] before thread 0 advances it).  Queries: the log of a stream is cut into chunks of
// AV_TAGLOG_CHUNK = 1024 frames, ONE WAVE per chunk (16 rounds of 64 lanes), four chunks per workgroup, grid (chunks / 4, S): a
// stream of 2^20 frames is 1024 waves, so S = 1 uses the whole device.  Waves never talk inside a launch; what a chunk needs of the
// chunks before it goes through the caller's workspace between launches:
//   match    (pass 1 of search and segments)  per chunk: the 1024 match bits (16 ballots), their count, the last non-matching index
//   search   (pass 2)   exclusive sum of the counts of the chunks before (every wave adds them up itself: no scan launch), then the
//                       ordered write from the BITS alone: the masks are read once, 8 B per frame
//   segments (pass 2)   prefix maximum of the last non-matching index = where a run that is open at the chunk's start began; a run
//                       is emitted from its END frame (bit on, next bit off), so every run belongs to exactly one chunk; counts kept runs
//            (pass 3)   the same walk, with the exclusive sum of the kept counts as the write position
//   stats    (pass 1)   per chunk a partial av_taglog_stats_row (64 ballot-popcount sums, wave min / max / sum of the speeds)
//            (pass 2)   one workgroup per stream folds the partials in a fixed order (so speed_sum is reproducible too)
// The exclusive sums re-read the per-chunk words of all earlier chunks: (cap / 1024)^2 / 2 int32 loads per stream and query, 2 MB
// out of L2 at 2^20 frames -- less than the masks; a log of 2^24 frames would want a scan launch instead.
// No LDS except the stats fold, no atomics, every store a plain vector store.
//
// Records.  A log may carry a third array, av_taglog_cols [S][cap] (80 B, array of structs): the numbers of the taggers' rows that a
// mask cannot hold.  av_tags_cols builds them (one lane per 8-byte word of a record, so the stores are contiguous; copies only),
// the append kernel moves them with the masks (a stream's window of records is one contiguous run of words), the match pass bounds
// them -- a bounded field costs one 8-byte load out of the frame's 80 B record, under a wave-uniform branch -- and
// av_taglog_gather turns a search's indices into records (one lane per output word).
//
// One kernel body per operation.  taglog_append_kernel<COLS> and taglog_match_kernel<BOUNDS> are each compiled twice: the <false>
// instance never forms a pointer into the speeds or records (40 VGPRs, 8 waves / SIMD for the match; 62 and 7 with the bounds,
// DESIGN 7k), and the host picks it when the query sets no numeric bound / the log has no records.  av_taglog_append, _search and
// _segments are av_taglog_append_ex, _search_where and _segments_where with the records and bounds absent.
#include "common.h"

#include <cmath>
#include <cstddef>

namespace {

constexpr int CHUNK = AV_TAGLOG_CHUNK;      // frames per wave
constexpr int ROUNDS = CHUNK / 64;          // 16
constexpr int STAT_FIELDS = 73;             // av_taglog_stats_row in 8-byte words
static_assert(sizeof(av_taglog_stats_row) == STAT_FIELDS * 8, "av_taglog_stats_row layout");
static_assert(ROUNDS <= 64 && CHUNK % 64 == 0, "one lane per round's ballot");

__host__ __device__ inline int n_chunks_of(int cap) { return (cap + CHUNK - 1) / CHUNK; }

// workspace: bits u64 [S][nc][16] | cnt i32 [S][nc] | lastoff i32 [S][nc] | kept i32 [S][nc] | pad to 8 | partial stats [S][nc][73] x 8 B
struct Workspace {
    unsigned long long* bits;
    int32_t *cnt, *lastoff, *kept;
    unsigned long long* part;
};
__host__ __device__ inline size_t ws_ints(size_t sc) { return (3 * sc + 1) & ~(size_t)1; }
__host__ __device__ inline Workspace carve(void* ws, int n_streams, int cap) {
    const size_t sc = (size_t)n_streams * (size_t)n_chunks_of(cap);
    Workspace w;
    w.bits = reinterpret_cast<unsigned long long*>(ws);
    w.cnt = reinterpret_cast<int32_t*>(w.bits + sc * ROUNDS);
    w.lastoff = w.cnt + sc;
    w.kept = w.lastoff + sc;
    w.part = reinterpret_cast<unsigned long long*>(w.cnt + ws_ints(sc));
    return w;
}

struct Predicate {
    unsigned long long all, any, none;
};
__device__ __forceinline__ bool matches(unsigned long long m, const Predicate& p) {
    return (m & p.all) == p.all && (p.any == 0ull || (m & p.any) != 0ull) && (m & p.none) == 0ull;
}

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// sum of a[0 .. c) over the wave (every wave adds up the chunks before its own)
__device__ __forceinline__ int sum_before(const int32_t* __restrict__ a, int c, int lane) {
    int v = 0;
    for (int j = lane; j < c; j += 64) v += a[j];
    return wave_sum_i(v);
}
// max of a[0 .. c) and -1; the entries are >= -1
__device__ __forceinline__ int max_before(const int32_t* __restrict__ a, int c, int lane) {
    unsigned v = 0;
    for (int j = lane; j < c; j += 64) {
        const unsigned x = (unsigned)(a[j] + 1);
        v = x > v ? x : v;
    }
    return (int)wave_max_u32(v) - 1;
}

// ---- pack ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long enum_bit(int v, int n, int base) {
    return (v >= 0 && v < n) ? (1ull << (base + v)) : 0ull;    // outside its range: no bit, never a neighbouring field's
}

__global__ void __launch_bounds__(256) tags_pack_kernel(int n_frames, const av_maneuver_row* __restrict__ maneuver,
                                                        const av_interaction_row* __restrict__ irows,
                                                        const av_interaction_summary* __restrict__ isum,
                                                        const int32_t* __restrict__ snap_n, int tcap,
                                                        const av_scene_row* __restrict__ scene, const int32_t* __restrict__ det_n,
                                                        const int32_t* __restrict__ det_cls, int max_det,
                                                        const uint8_t* __restrict__ elem, int n_elem,
                                                        unsigned long long* __restrict__ out_mask, double* __restrict__ out_speed) {
    const int lane = threadIdx.x & 63;
    const long long fl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (fl >= n_frames) return;
    const size_t f = (size_t)fl;
    unsigned lo = 0, hi = 0;                    // the lanes' parts: element bits (6..10) are low, interaction types (33..45) high
    unsigned long long m = 0;                   // the frame's own fields, the same in every lane
    double speed = __longlong_as_double(0x7ff8000000000000ll);
    if (scene) {
        const av_scene_row& r = scene[f];
        m |= 1ull << AV_TAG_HAS_SCENE;
        m |= enum_bit(r.road_type, 6, AV_TAG_ROAD_TYPE);
        int nc = r.n_conditions;
        nc = nc < 0 ? 0 : (nc > 3 ? 3 : nc);
        for (int k = 0; k < nc; ++k) m |= enum_bit(r.conditions[k], 6, AV_TAG_CONDITION);
        if (r.has_pedestrian != 0) m |= 1ull << AV_TAG_PEDESTRIAN_AREA;
        if (det_n) {
            int n = det_n[f];
            n = n < 0 ? 0 : (n > max_det ? max_det : n);
            const int32_t* cls = det_cls + f * (size_t)max_det;
            for (int b = 0; b < n; b += 64) {
                const int i = b + lane;
                if (i < n) {
                    const int c = cls[i];
                    const int e = (c >= 0 && c < n_elem) ? (int)elem[c] : 0;       // TrafficElement index + 1
                    if (e >= 1 && e <= 5) lo |= 1u << (AV_TAG_ELEMENT + e - 1);
                }
            }
        }
    }
    if (maneuver) {
        const av_maneuver_row& r = maneuver[f];
        m |= 1ull << AV_TAG_HAS_MANEUVER;
        m |= enum_bit(r.lateral, 4, AV_TAG_LATERAL) | enum_bit(r.longitudinal, 5, AV_TAG_LONGITUDINAL) |
             enum_bit(r.turning, 6, AV_TAG_TURNING);
        speed = r.speed_kmh;
    }
    if (isum) {
        m |= 1ull << AV_TAG_HAS_INTERACTION;
        const int risk = isum[f].overall_risk;
        if (risk >= 1 && risk <= 3) m |= 1ull << (AV_TAG_RISK + risk - 1);
        int n = tcap;                                                              // av_tags_pack_slots: every row
        if (snap_n) {
            n = snap_n[f];
            n = n < 0 ? 0 : (n > tcap ? tcap : n);
        }
        for (int b = 0; b < n; b += 64) {                                          // (av_tags_pack's tcap is 64: one round)
            const int i = b + lane;
            if (i < n) {
                const av_interaction_row& r = irows[f * (size_t)tcap + i];
                if (r.type >= 0 && r.type < 13 && r.confidence > 0.5) hi |= 1u << (AV_TAG_INTERACTION - 32 + r.type);
            }
        }
    }
    lo = wave_or_u32(lo);
    hi = wave_or_u32(hi);
    if (lane == 0) {
        out_mask[f] = m | ((unsigned long long)hi << 32) | lo;
        out_speed[f] = speed;
    }
}

// ---- records ---------------------------------------------------------------------------------------------------------------
constexpr int COLS_WORDS = 10;              // av_taglog_cols in 8-byte words
static_assert(sizeof(av_taglog_cols) == COLS_WORDS * 8, "av_taglog_cols layout");
static_assert(sizeof(av_taglog_where) == 88, "av_taglog_where layout");
static_assert(offsetof(av_taglog_cols, acceleration) == 32 && offsetof(av_taglog_cols, min_ttc) == 48 &&
              offsetof(av_taglog_cols, closest_distance) == 56 && offsetof(av_taglog_cols, agent_count) == 64 &&
              offsetof(av_taglog_cols, cyclist_count) == 72, "av_taglog_cols words");
static_assert(offsetof(av_maneuver_row, lateral_confidence) == 16 && offsetof(av_maneuver_row, turning_confidence) == 32 &&
              offsetof(av_maneuver_row, acceleration) == 48 && offsetof(av_maneuver_row, yaw_rate_deg) == 56 &&
              sizeof(av_maneuver_row) == 72, "av_maneuver_row words");
static_assert(offsetof(av_interaction_summary, agent_count) == 0 && offsetof(av_interaction_summary, cyclist_count) == 8 &&
              offsetof(av_interaction_summary, closest_distance) == 32 && offsetof(av_interaction_summary, min_ttc) == 40 &&
              sizeof(av_interaction_summary) == 56, "av_interaction_summary words");
static_assert(offsetof(av_scene_row, confidence) % 8 == 0 && sizeof(av_scene_row) % 8 == 0, "av_scene_row words");
constexpr unsigned long long NAN_BITS = 0x7ff8000000000000ull;
constexpr int W_ACCEL = 4, W_TTC = 6, W_DIST = 7, W_AGENT_PED = 8, W_CYC_VEH = 9;      // words of a record the queries read

// word -> word of the source row, in 8-byte words (the two count words are two int32 each, in the summary's order)
__global__ void __launch_bounds__(256) tags_cols_kernel(long long n_words, const unsigned long long* __restrict__ maneuver,
                                                        const unsigned long long* __restrict__ isum,
                                                        const unsigned long long* __restrict__ scene,
                                                        unsigned long long* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_words) return;
    const size_t f = (size_t)(t / COLS_WORDS);
    const int w = (int)(t % COLS_WORDS);
    unsigned long long v = 0ull;
    if (w == 0) {
        if (scene) v = scene[f * (sizeof(av_scene_row) / 8) + offsetof(av_scene_row, confidence) / 8];
    } else if (w < 6) {                     // 1..3 the confidences (row words 2..4), 4..5 acceleration, yaw_rate_deg (6..7)
        if (maneuver) v = maneuver[f * (sizeof(av_maneuver_row) / 8) + (w < 4 ? w + 1 : w + 2)];
    } else if (w < 8) {                     // min_ttc (summary word 5), closest_distance (4)
        v = isum ? isum[f * (sizeof(av_interaction_summary) / 8) + (w == W_TTC ? 5 : 4)] : NAN_BITS;
    } else {                                // agent | pedestrian (word 0), cyclist | vehicle (word 1)
        if (isum) v = isum[f * (sizeof(av_interaction_summary) / 8) + (w - 8)];
    }
    out[t] = v;
}

// ---- append ----------------------------------------------------------------------------------------------------------------
// COLS: with the records; a stream's `fit` records are fit * 10 consecutive words on both sides.
template <bool COLS>
__global__ void __launch_bounds__(256) taglog_append_kernel(int n_frames, const unsigned long long* __restrict__ mask,
                                                            const double* __restrict__ speed, int cap,
                                                            unsigned long long* __restrict__ log_mask, double* __restrict__ log_speed,
                                                            int32_t* __restrict__ log_n, int32_t* __restrict__ dropped,
                                                            const unsigned long long* __restrict__ cols,
                                                            unsigned long long* __restrict__ log_cols) {
    const size_t s = blockIdx.x;
    int n0 = log_n[s];
    n0 = n0 < 0 ? 0 : (n0 > cap ? cap : n0);
    __syncthreads();                            // every thread has read log_n[s] before thread 0 advances it
    const int fit = n_frames < cap - n0 ? n_frames : cap - n0;
    for (int w = threadIdx.x; w < fit; w += blockDim.x) {                          // n0 + w < n0 + fit <= cap
        log_mask[s * (size_t)cap + n0 + w] = mask[s * (size_t)n_frames + w];
        log_speed[s * (size_t)cap + n0 + w] = speed[s * (size_t)n_frames + w];
    }
    if constexpr (COLS) {
        const unsigned long long* src = cols + s * (size_t)n_frames * COLS_WORDS;
        unsigned long long* dst = log_cols + (s * (size_t)cap + (size_t)n0) * COLS_WORDS;
        const long long words = (long long)fit * COLS_WORDS;                       // (n0 + fit) * 10 <= cap * 10 words of the row
        for (long long j = threadIdx.x; j < words; j += blockDim.x) dst[j] = src[j];
    }
    if (threadIdx.x == 0) {
        log_n[s] = n0 + fit;
        dropped[s] += n_frames - fit;
    }
}

// One lane per output word of a gathered row: word 0 the mask, 1 the speed, 2..11 the record.
constexpr int GATHER_WORDS = 2 + COLS_WORDS;
__global__ void __launch_bounds__(256) taglog_gather_kernel(int cap, const unsigned long long* __restrict__ log_mask,
                                                            const unsigned long long* __restrict__ log_speed,
                                                            const unsigned long long* __restrict__ log_cols,
                                                            const int32_t* __restrict__ log_n, const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ idx_n, int idx_cap,
                                                            unsigned long long* __restrict__ out_mask,
                                                            unsigned long long* __restrict__ out_speed,
                                                            unsigned long long* __restrict__ out_cols) {
    const size_t s = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = t / GATHER_WORDS;
    const int w = (int)(t % GATHER_WORDS);
    int rows = idx_n[s];
    rows = rows < 0 ? 0 : (rows > idx_cap ? idx_cap : rows);
    if (row >= rows || (w >= 2 && !log_cols)) return;                              // row < rows <= idx_cap
    int n = log_n[s];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const int f = idx[s * (size_t)idx_cap + (size_t)row];
    const bool in = f >= 0 && f < n;                                               // f < n <= cap: inside the stream's row
    const size_t src = s * (size_t)cap + (size_t)(in ? f : 0), dst = s * (size_t)idx_cap + (size_t)row;
    if (w == 0) out_mask[dst] = in ? log_mask[src] : 0ull;
    else if (w == 1) out_speed[dst] = in ? log_speed[src] : 0ull;
    else out_cols[dst * COLS_WORDS + (w - 2)] = in ? log_cols[src * COLS_WORDS + (w - 2)] : 0ull;
}

// ---- queries: the wave's chunk ---------------------------------------------------------------------------------------------
struct ChunkId {
    int lane, c, nc;
    size_t s, sc;           // stream, stream * nc + c
    bool live;
};
__device__ __forceinline__ ChunkId my_chunk(int cap) {
    ChunkId k;
    k.lane = threadIdx.x & 63;
    k.nc = n_chunks_of(cap);
    k.c = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    k.s = blockIdx.y;
    k.live = k.c < k.nc;
    k.sc = k.s * (size_t)k.nc + (size_t)(k.live ? k.c : 0);
    return k;
}

// Pass 1 of search and segments: a chunk's bits / cnt / lastoff from the masks and, BOUNDS, from speeds and records.  Which arrays
// are read is decided by the bounds that are set -- kernel arguments, so every such branch is wave-uniform.
struct WhereUse {
    bool speed, accel, ttc, dist, agent_ped, cyc_veh;
    __host__ __device__ bool any() const { return speed || accel || ttc || dist || agent_ped || cyc_veh; }
};
__host__ __device__ inline bool is_set(double bound) { return bound == bound; }
__host__ __device__ inline WhereUse where_use(const av_taglog_where& q) {
    WhereUse u;
    u.speed = is_set(q.speed_min) || is_set(q.speed_max);
    u.accel = is_set(q.accel_min) || is_set(q.accel_max);
    u.ttc = is_set(q.ttc_max);
    u.dist = is_set(q.distance_max);
    u.agent_ped = q.agents_min > 0 || q.pedestrians_min > 0;
    u.cyc_veh = q.cyclists_min > 0 || q.vehicles_min > 0;
    return u;
}
// an unset (NaN) bound imposes nothing; a set one is false against a stored NaN
__device__ __forceinline__ bool at_least(double v, double bound) { return !is_set(bound) || v >= bound; }
__device__ __forceinline__ bool at_most(double v, double bound) { return !is_set(bound) || v <= bound; }
__device__ __forceinline__ bool count_at_least(int v, int bound) { return bound <= 0 || v >= bound; }

template <bool BOUNDS>
__global__ void __launch_bounds__(256) taglog_match_kernel(int cap, const unsigned long long* __restrict__ log_mask,
                                                           const double* __restrict__ log_speed,
                                                           const unsigned long long* __restrict__ log_cols,
                                                           const int32_t* __restrict__ log_n, av_taglog_where q, int first, int last,
                                                           Workspace ws) {
    const ChunkId k = my_chunk(cap);
    if (!k.live) return;
    int n = log_n[k.s];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const int lo = first < 0 ? 0 : first, hi = last < n ? last : n;
    const int base = k.c * CHUNK;
    const Predicate p{q.all, q.any, q.none};
    const WhereUse use = where_use(q);
    const unsigned long long* row = log_mask + k.s * (size_t)cap;
    // <false> forms neither pointer and reads no bound (DESIGN 7k on why they stand here and not inside the `if constexpr`)
    const double* vrow = BOUNDS ? log_speed + k.s * (size_t)cap : nullptr;
    const unsigned long long* crow = BOUNDS ? log_cols + k.s * (size_t)cap * COLS_WORDS : nullptr;
    unsigned long long mine = 0;                // lane r keeps round r's ballot
    int count = 0, lastoff = -1;
    if (base < hi && base + CHUNK > lo) {       // otherwise nothing of this chunk is in range: all bits off, no load
        unsigned long long m[ROUNDS];           // the masks first: 16 loads in flight
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int i = base + r * 64 + k.lane;
            m[r] = (i >= lo && i < hi) ? row[i] : 0ull;                            // i < hi <= n <= cap
        }
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int i = base + r * 64 + k.lane;
            const bool in = i >= lo && i < hi;                                     // every load below: i < hi <= n <= cap
            bool ok = in && matches(m[r], p);
            if constexpr (BOUNDS) {
                const unsigned long long* rec = crow + (size_t)(in ? i : 0) * COLS_WORDS;      // read under `in` only
                if (use.speed) {
                    const double v = in ? vrow[i] : 0.0;
                    ok = ok && at_least(v, q.speed_min) && at_most(v, q.speed_max);
                }
                if (use.accel) {
                    const double v = __longlong_as_double((long long)(in ? rec[W_ACCEL] : 0ull));
                    ok = ok && at_least(v, q.accel_min) && at_most(v, q.accel_max);
                }
                if (use.ttc) ok = ok && at_most(__longlong_as_double((long long)(in ? rec[W_TTC] : 0ull)), q.ttc_max);
                if (use.dist) ok = ok && at_most(__longlong_as_double((long long)(in ? rec[W_DIST] : 0ull)), q.distance_max);
                if (use.agent_ped) {
                    const unsigned long long v = in ? rec[W_AGENT_PED] : 0ull;
                    ok = ok && count_at_least((int)(unsigned)v, q.agents_min) && count_at_least((int)(unsigned)(v >> 32), q.pedestrians_min);
                }
                if (use.cyc_veh) {
                    const unsigned long long v = in ? rec[W_CYC_VEH] : 0ull;
                    ok = ok && count_at_least((int)(unsigned)v, q.cyclists_min) && count_at_least((int)(unsigned)(v >> 32), q.vehicles_min);
                }
            }
            const unsigned long long on = __ballot(ok);
            if (k.lane == r) mine = on;
            count += __popcll(on);
            if (~on != 0ull) lastoff = base + r * 64 + 63 - __clzll(~on);
        }
    } else {
        lastoff = base + CHUNK - 1;
    }
    if (k.lane < ROUNDS) ws.bits[k.sc * ROUNDS + k.lane] = mine;
    if (k.lane == 0) ws.cnt[k.sc] = count, ws.lastoff[k.sc] = lastoff;
}

__global__ void __launch_bounds__(256) taglog_search_write_kernel(int cap, Workspace ws, int out_cap, int32_t* __restrict__ out_idx,
                                                                  int32_t* __restrict__ out_n) {
    const ChunkId k = my_chunk(cap);
    if (!k.live) return;
    const int own = ws.cnt[k.sc];
    int run = sum_before(ws.cnt + k.s * (size_t)k.nc, k.c, k.lane);
    if (k.c == k.nc - 1 && k.lane == 0) out_n[k.s] = run + own;
    if (own == 0 || run >= out_cap) return;
    const unsigned long long mine = k.lane < ROUNDS ? ws.bits[k.sc * ROUNDS + k.lane] : 0ull;
    int32_t* out = out_idx + k.s * (size_t)out_cap;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const unsigned long long on = readlane_u64(mine, r);
        const int pos = run + __popcll(on & lanes_below(k.lane));
        if (((on >> k.lane) & 1ull) && pos < out_cap) out[pos] = k.c * CHUNK + r * 64 + k.lane;
        run += __popcll(on);
    }
}

// Pass 2 (WRITE false: kept[chunk]) and pass 3 (WRITE true) of the segment query.
template <bool WRITE>
__global__ void __launch_bounds__(256) taglog_segments_kernel(int cap, Workspace ws, int min_duration, int seg_cap,
                                                              int32_t* __restrict__ out_seg, int32_t* __restrict__ out_n) {
    const ChunkId k = my_chunk(cap);
    if (!k.live) return;
    const size_t s0 = k.s * (size_t)k.nc;
    int run = 0;
    if (WRITE) {
        run = sum_before(ws.kept + s0, k.c, k.lane);
        const int own = ws.kept[k.sc];
        if (k.c == k.nc - 1 && k.lane == 0) out_n[k.s] = run + own;
        if (own == 0 || run >= seg_cap) return;
    } else if (ws.cnt[k.sc] == 0) {             // no matching frame, so no run ends here
        if (k.lane == 0) ws.kept[k.sc] = 0;
        return;
    }
    int carry = max_before(ws.lastoff + s0, k.c, k.lane);          // the last non-matching frame before this chunk (-1: none)
    const unsigned long long mine = k.lane < ROUNDS ? ws.bits[k.sc * ROUNDS + k.lane] : 0ull;
    // the bit after the chunk's last: the first of the next chunk (off past the end of the grid; frames outside the range are off)
    const unsigned long long after = k.c + 1 < k.nc ? (ws.bits[(k.sc + 1) * ROUNDS] & 1ull) : 0ull;
    const int base = k.c * CHUNK;
    int32_t* out = out_seg + k.s * (size_t)seg_cap * 2;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const unsigned long long on = readlane_u64(mine, r);
        const unsigned long long next0 = r + 1 < ROUNDS ? (readlane_u64(mine, r + 1 < ROUNDS ? r + 1 : r) & 1ull) : after;
        const unsigned long long ends = on & ~((on >> 1) | (next0 << 63));
        const unsigned long long off_below = ~on & lanes_below(k.lane);
        const int i = base + r * 64 + k.lane;
        const int start = off_below ? base + r * 64 + 64 - __clzll(off_below) : carry + 1;
        const bool keep = ((ends >> k.lane) & 1ull) && (i - start + 1 >= min_duration);
        const unsigned long long kb = __ballot(keep);
        if (WRITE) {
            const int pos = run + __popcll(kb & lanes_below(k.lane));
            if (keep && pos < seg_cap) out[(size_t)pos * 2] = start, out[(size_t)pos * 2 + 1] = i;
        }
        run += __popcll(kb);
        if (~on != 0ull) carry = base + r * 64 + 63 - __clzll(~on);
    }
    if (!WRITE && k.lane == 0) ws.kept[k.sc] = run;
}

// ---- stats -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_fmin(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double wave_fmax(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

__global__ void __launch_bounds__(256) taglog_stats_chunk_kernel(int cap, const unsigned long long* __restrict__ log_mask,
                                                                 const double* __restrict__ log_speed,
                                                                 const int32_t* __restrict__ log_n, Workspace ws) {
    const ChunkId k = my_chunk(cap);
    if (!k.live) return;
    int n = log_n[k.s];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const int base = k.c * CHUNK;
    unsigned long long* part = ws.part + k.sc * STAT_FIELDS;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    long long tag = 0, frames = 0, man = 0, r0 = 0, r1 = 0, r2 = 0, r3 = 0;
    double smin = inf, smax = -inf, ssum = 0.0;
    if (base < n) {
        unsigned long long m[ROUNDS];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int i = base + r * 64 + k.lane;
            m[r] = i < n ? log_mask[k.s * (size_t)cap + i] : 0ull;                 // i < n <= cap
            const bool has = (m[r] >> AV_TAG_HAS_MANEUVER) & 1ull;
            if (has) {
                const double v = log_speed[k.s * (size_t)cap + i];
                smin = fmin(smin, v), smax = fmax(smax, v), ssum += v;
            }
            const int left = n - (base + r * 64);
            frames += left >= 64 ? 64 : (left > 0 ? left : 0);
            man += __popcll(__ballot(has));
            const bool inter = (m[r] >> AV_TAG_HAS_INTERACTION) & 1ull;
            const unsigned risk = (unsigned)(m[r] >> AV_TAG_RISK) & 7u;
            r0 += __popcll(__ballot(inter && risk == 0u));
            r1 += __popcll(__ballot((risk & 1u) != 0u));
            r2 += __popcll(__ballot((risk & 2u) != 0u));
            r3 += __popcll(__ballot((risk & 4u) != 0u));
        }
#pragma unroll 1
        for (int b = 0; b < 64; ++b) {          // frames carrying bit b: lane b keeps the sum
            int c = 0;
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) c += __popcll(__ballot((m[r] >> b) & 1ull));
            if (k.lane == b) tag = c;
        }
        smin = wave_fmin(smin), smax = wave_fmax(smax), ssum = wave_sum_dpp(ssum);
    }
    part[k.lane] = (unsigned long long)tag;
    if (k.lane == 0) {
        part[64] = (unsigned long long)frames, part[65] = (unsigned long long)man;
        part[66] = (unsigned long long)r0, part[67] = (unsigned long long)r1, part[68] = (unsigned long long)r2,
        part[69] = (unsigned long long)r3;
        part[70] = (unsigned long long)__double_as_longlong(smin), part[71] = (unsigned long long)__double_as_longlong(smax);
        part[72] = (unsigned long long)__double_as_longlong(ssum);
    }
}

// field f of two partial rows folded: 0..69 integer sums, 70 min, 71 max, 72 sum
__device__ __forceinline__ unsigned long long fold(int f, unsigned long long a, unsigned long long b) {
    if (f < 70) return a + b;
    const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
    const double z = f == 70 ? fmin(x, y) : (f == 71 ? fmax(x, y) : x + y);
    return (unsigned long long)__double_as_longlong(z);
}
__device__ __forceinline__ unsigned long long fold_identity(int f) {
    return f == 70 ? 0x7ff0000000000000ull : (f == 71 ? 0xfff0000000000000ull : 0ull);
}

constexpr int FOLD_WAVES = 16;
__global__ void __launch_bounds__(FOLD_WAVES * 64) taglog_stats_fold_kernel(int cap, Workspace ws, av_taglog_stats_row* __restrict__ out) {
    __shared__ unsigned long long acc[FOLD_WAVES][STAT_FIELDS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nc = n_chunks_of(cap);
    const size_t s = blockIdx.x;
    const unsigned long long* part = ws.part + s * (size_t)nc * STAT_FIELDS;
    const int f2 = 64 + lane;                   // a lane folds field `lane` and, the first nine, field 64 + lane
    unsigned long long a = 0ull, b = fold_identity(f2 < STAT_FIELDS ? f2 : 0);
    for (int c = wv; c < nc; c += FOLD_WAVES) {                    // wave wv: chunks wv, wv + 16, ... in order
        a += part[(size_t)c * STAT_FIELDS + lane];
        if (f2 < STAT_FIELDS) b = fold(f2, b, part[(size_t)c * STAT_FIELDS + f2]);
    }
    acc[wv][lane] = a;
    if (f2 < STAT_FIELDS) acc[wv][f2] = b;
    __syncthreads();
    for (int f = threadIdx.x; f < STAT_FIELDS; f += blockDim.x) {
        unsigned long long v = acc[0][f];
        for (int w = 1; w < FOLD_WAVES; ++w) v = fold(f, v, acc[w][f]);
        reinterpret_cast<unsigned long long*>(out + s)[f] = v;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
inline dim3 chunk_grid(int n_streams, int cap) { return dim3((unsigned)((n_chunks_of(cap) + 3) / 4), (unsigned)n_streams); }
inline const unsigned long long* words(const void* p) { return reinterpret_cast<const unsigned long long*>(p); }
inline unsigned long long* words(void* p) { return reinterpret_cast<unsigned long long*>(p); }

// what a log's arrays and a query over them are, as the entry points receive them
struct Query {
    const char* who;                            // the entry that was called, for its error texts
    av_ctx* ctx;
    av_stream_t stream;
    int n_streams, cap;
    const uint64_t* log_mask;
    const double* log_speed;
    const av_taglog_cols* log_cols;
    const int32_t* log_n;
    const av_taglog_where* where;
    int first, last;
    void* workspace;
};
// the mask-only entries' predicate: no numeric bound set
inline av_taglog_where masks_only(uint64_t all, uint64_t any, uint64_t none) {
    const double unset = __builtin_nan("");
    return av_taglog_where{all, any, none, unset, unset, unset, unset, unset, unset, 0, 0, 0, 0};
}

// Pass 1 of every query, behind the checks all of them share; 0 or the error code.  out / out_cap / out_n: the query's output.
int launch_match(const Query& q, int out_cap, const void* out, const int32_t* out_n) {
    AV_REQUIRE(q.ctx && q.log_mask && q.log_n && q.where && q.workspace && out_n && (out || out_cap == 0), AV_EINVAL,
               "%s: null argument", q.who);
    AV_REQUIRE(q.n_streams > 0 && q.cap > 0, AV_EINVAL, "%s: n_streams and cap must be > 0", q.who);
    AV_REQUIRE(out_cap >= 0, AV_EINVAL, "%s: the output capacity %d is negative", q.who, out_cap);
    const WhereUse use = where_use(*q.where);
    AV_REQUIRE(q.log_speed || !use.speed, AV_EINVAL, "%s: a speed bound without log_speed", q.who);
    AV_REQUIRE(q.log_cols || !(use.accel || use.ttc || use.dist || use.agent_ped || use.cyc_veh), AV_EINVAL,
               "%s: a bound on a record's field without log_cols", q.who);
    const auto kernel = use.any() ? taglog_match_kernel<true> : taglog_match_kernel<false>;
    hipLaunchKernelGGL(kernel, chunk_grid(q.n_streams, q.cap), dim3(256), 0, as_stream(q.stream), q.cap, words(q.log_mask), q.log_speed,
                       words(q.log_cols), q.log_n, *q.where, q.first, q.last, carve(q.workspace, q.n_streams, q.cap));
    AV_LAUNCH_CHECK();
    return AV_OK;
}

// match, then the ordered write
int run_search(const Query& q, int out_cap, int32_t* out_idx, int32_t* out_n) {
    const int rc = launch_match(q, out_cap, out_idx, out_n);
    if (rc != AV_OK) return rc;
    hipLaunchKernelGGL(taglog_search_write_kernel, chunk_grid(q.n_streams, q.cap), dim3(256), 0, as_stream(q.stream), q.cap,
                       carve(q.workspace, q.n_streams, q.cap), out_cap, out_idx, out_n);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

// match, count the kept runs per chunk, write them
int run_segments(const Query& q, int min_duration, int seg_cap, int32_t* out_seg, int32_t* out_n) {
    const int rc = launch_match(q, seg_cap, out_seg, out_n);
    if (rc != AV_OK) return rc;
    const Workspace ws = carve(q.workspace, q.n_streams, q.cap);
    const dim3 grid = chunk_grid(q.n_streams, q.cap);
    hipLaunchKernelGGL(taglog_segments_kernel<false>, grid, dim3(256), 0, as_stream(q.stream), q.cap, ws, min_duration, seg_cap, out_seg,
                       out_n);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(taglog_segments_kernel<true>, grid, dim3(256), 0, as_stream(q.stream), q.cap, ws, min_duration, seg_cap, out_seg,
                       out_n);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int run_append(const char* who, av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const uint64_t* mask, const double* speed,
               const av_taglog_cols* cols, int cap, uint64_t* log_mask, double* log_speed, av_taglog_cols* log_cols, int32_t* log_n,
               int32_t* dropped) {
    AV_REQUIRE(ctx && mask && speed && log_mask && log_speed && log_n && dropped, AV_EINVAL, "%s: null argument", who);
    AV_REQUIRE((cols == nullptr) == (log_cols == nullptr), AV_EINVAL, "%s: cols and log_cols are given together or not at all", who);
    AV_REQUIRE(n_streams > 0 && n_frames > 0 && cap > 0, AV_EINVAL, "%s: n_streams, n_frames and cap must be > 0", who);
    const auto kernel = cols ? taglog_append_kernel<true> : taglog_append_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_streams), dim3(256), 0, as_stream(stream), n_frames, words(mask), speed, cap, words(log_mask),
                       log_speed, log_n, dropped, words(cols), words(log_cols));
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // namespace

extern "C" size_t av_taglog_workspace_bytes(int n_streams, int cap) {
    if (n_streams <= 0 || cap <= 0) return 0;
    const size_t sc = (size_t)n_streams * (size_t)n_chunks_of(cap);
    return sc * ROUNDS * 8 + ws_ints(sc) * 4 + sc * STAT_FIELDS * 8;
}

extern "C" int av_tags_pack(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const av_maneuver_row* maneuver,
                            const av_interaction_row* inter_rows, const av_interaction_summary* inter_summary,
                            const int32_t* snap_n, int tcap, const av_scene_row* scene, const int32_t* det_n, const int32_t* det_cls,
                            int max_det, const uint8_t* elem_table, int n_elem, uint64_t* out_mask, double* out_speed) {
    AV_REQUIRE(ctx && out_mask && out_speed, AV_EINVAL, "av_tags_pack: null argument");
    AV_REQUIRE(n_streams > 0 && n_frames > 0, AV_EINVAL, "av_tags_pack: n_streams and n_frames must be > 0");
    const bool inter = inter_rows || inter_summary || snap_n;
    AV_REQUIRE(!inter || (inter_rows && inter_summary && snap_n), AV_EINVAL,
               "av_tags_pack: inter_rows, inter_summary and snap_n are given together or not at all");
    AV_REQUIRE(!inter || tcap == 64, AV_EINVAL, "av_tags_pack: tcap %d, the interaction rows come 64 to a frame", tcap);
    const bool det = det_n || det_cls || elem_table;
    AV_REQUIRE(!det || (det_n && det_cls && elem_table), AV_EINVAL,
               "av_tags_pack: det_n, det_cls and elem_table are given together or not at all");
    AV_REQUIRE(!det || scene, AV_EINVAL, "av_tags_pack: detections without scene rows (traffic elements are scene tags)");
    AV_REQUIRE(!det || (max_det > 0 && n_elem >= 0), AV_EINVAL, "av_tags_pack: max_det must be > 0 and n_elem >= 0");
    const long long frames = (long long)n_streams * n_frames;
    AV_REQUIRE(frames <= 0x7fffffffll, AV_EINVAL, "av_tags_pack: n_streams * n_frames does not fit an int");
    hipLaunchKernelGGL(tags_pack_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, as_stream(stream), (int)frames, maneuver,
                       inter_rows, inter_summary, snap_n, tcap, scene, det_n, det_cls, max_det, elem_table, n_elem,
                       words(out_mask), out_speed);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_tags_pack_slots(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const av_maneuver_row* maneuver,
                                  const av_interaction_row* inter_rows, const av_interaction_summary* inter_summary, int tcap,
                                  uint64_t* out_mask, double* out_speed) {
    AV_REQUIRE(n_streams > 0 && n_frames > 0, AV_EINVAL, "av_tags_pack_slots: n_streams and n_frames must be > 0");
    AV_REQUIRE((inter_rows != nullptr) == (inter_summary != nullptr), AV_EINVAL,
               "av_tags_pack_slots: inter_rows and inter_summary are given together or not at all");
    AV_REQUIRE(!inter_rows || (tcap >= 1 && tcap <= 512), AV_EINVAL, "av_tags_pack_slots: tcap %d not in 1..512", tcap);
    const long long frames = (long long)n_streams * n_frames;
    AV_REQUIRE(frames <= 0x7fffffffll, AV_EINVAL, "av_tags_pack_slots: n_streams * n_frames does not fit an int");
    AV_REQUIRE(ctx && out_mask && out_speed, AV_EINVAL, "av_tags_pack_slots: null argument");
    hipLaunchKernelGGL(tags_pack_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, as_stream(stream), (int)frames, maneuver,
                       inter_rows, inter_summary, nullptr, tcap, nullptr, nullptr, nullptr, 0, nullptr, 0, words(out_mask), out_speed);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_taglog_append(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const uint64_t* mask,
                                const double* speed, int cap, uint64_t* log_mask, double* log_speed, int32_t* log_n,
                                int32_t* dropped) {
    return run_append("av_taglog_append", ctx, stream, n_streams, n_frames, mask, speed, nullptr, cap, log_mask, log_speed, nullptr, log_n,
                      dropped);
}

extern "C" int av_taglog_append_ex(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const uint64_t* mask,
                                   const double* speed, const av_taglog_cols* cols, int cap, uint64_t* log_mask, double* log_speed,
                                   av_taglog_cols* log_cols, int32_t* log_n, int32_t* dropped) {
    return run_append("av_taglog_append_ex", ctx, stream, n_streams, n_frames, mask, speed, cols, cap, log_mask, log_speed, log_cols,
                      log_n, dropped);
}

extern "C" int av_taglog_search(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask,
                                const int32_t* log_n, uint64_t all, uint64_t any, uint64_t none, int first, int last, void* workspace,
                                int out_cap, int32_t* out_idx, int32_t* out_n) {
    const av_taglog_where where = masks_only(all, any, none);
    return run_search({"av_taglog_search", ctx, stream, n_streams, cap, log_mask, nullptr, nullptr, log_n, &where, first, last, workspace},
                      out_cap, out_idx, out_n);
}

extern "C" int av_taglog_search_where(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask,
                                      const double* log_speed, const av_taglog_cols* log_cols, const int32_t* log_n,
                                      const av_taglog_where* where, int first, int last, void* workspace, int out_cap,
                                      int32_t* out_idx, int32_t* out_n) {
    return run_search({"av_taglog_search_where", ctx, stream, n_streams, cap, log_mask, log_speed, log_cols, log_n, where, first, last,
                       workspace}, out_cap, out_idx, out_n);
}

extern "C" int av_taglog_segments(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask,
                                  const int32_t* log_n, uint64_t all, uint64_t any, uint64_t none, int first, int last,
                                  int min_duration, void* workspace, int seg_cap, int32_t* out_seg, int32_t* out_n) {
    const av_taglog_where where = masks_only(all, any, none);
    return run_segments({"av_taglog_segments", ctx, stream, n_streams, cap, log_mask, nullptr, nullptr, log_n, &where, first, last,
                         workspace}, min_duration, seg_cap, out_seg, out_n);
}

extern "C" int av_taglog_segments_where(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask,
                                        const double* log_speed, const av_taglog_cols* log_cols, const int32_t* log_n,
                                        const av_taglog_where* where, int first, int last, int min_duration, void* workspace,
                                        int seg_cap, int32_t* out_seg, int32_t* out_n) {
    return run_segments({"av_taglog_segments_where", ctx, stream, n_streams, cap, log_mask, log_speed, log_cols, log_n, where, first,
                         last, workspace}, min_duration, seg_cap, out_seg, out_n);
}

extern "C" int av_taglog_stats(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask,
                               const double* log_speed, const int32_t* log_n, void* workspace, av_taglog_stats_row* out) {
    AV_REQUIRE(ctx && log_mask && log_speed && log_n && workspace && out, AV_EINVAL, "av_taglog_stats: null argument");
    AV_REQUIRE(n_streams > 0 && cap > 0, AV_EINVAL, "av_taglog_stats: n_streams and cap must be > 0");
    const Workspace ws = carve(workspace, n_streams, cap);
    hipLaunchKernelGGL(taglog_stats_chunk_kernel, chunk_grid(n_streams, cap), dim3(256), 0, as_stream(stream), cap,
                       words(log_mask), log_speed, log_n, ws);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(taglog_stats_fold_kernel, dim3((unsigned)n_streams), dim3(FOLD_WAVES * 64), 0, as_stream(stream), cap, ws, out);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_tags_cols(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, const av_maneuver_row* maneuver,
                            const av_interaction_summary* inter_summary, const av_scene_row* scene, av_taglog_cols* out_cols) {
    AV_REQUIRE(ctx && out_cols, AV_EINVAL, "av_tags_cols: null argument");
    AV_REQUIRE(n_streams > 0 && n_frames > 0, AV_EINVAL, "av_tags_cols: n_streams and n_frames must be > 0");
    const long long frames = (long long)n_streams * n_frames;
    AV_REQUIRE(frames <= 0x7fffffffll / COLS_WORDS, AV_EINVAL, "av_tags_cols: n_streams * n_frames * 10 does not fit an int");
    const long long n_words = frames * COLS_WORDS;
    hipLaunchKernelGGL(tags_cols_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, as_stream(stream), n_words,
                       words(maneuver), words(inter_summary), words(scene), words(out_cols));
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_taglog_gather(av_ctx* ctx, av_stream_t stream, int n_streams, int cap, const uint64_t* log_mask,
                                const double* log_speed, const av_taglog_cols* log_cols, const int32_t* log_n, const int32_t* idx,
                                const int32_t* idx_n, int idx_cap, uint64_t* out_mask, double* out_speed, av_taglog_cols* out_cols) {
    AV_REQUIRE(ctx && log_mask && log_speed && log_n && idx_n && out_mask && out_speed, AV_EINVAL, "av_taglog_gather: null argument");
    AV_REQUIRE(!log_cols || out_cols, AV_EINVAL, "av_taglog_gather: log_cols without out_cols");
    AV_REQUIRE(n_streams > 0 && cap > 0, AV_EINVAL, "av_taglog_gather: n_streams and cap must be > 0");
    AV_REQUIRE(idx_cap >= 0 && idx_cap <= 0x7fffffff / GATHER_WORDS, AV_EINVAL, "av_taglog_gather: idx_cap %d out of range", idx_cap);
    AV_REQUIRE(idx || idx_cap == 0, AV_EINVAL, "av_taglog_gather: null argument");
    if (idx_cap == 0) return AV_OK;
    const long long threads = (long long)idx_cap * GATHER_WORDS;
    hipLaunchKernelGGL(taglog_gather_kernel, dim3((unsigned)((threads + 255) / 256), (unsigned)n_streams), dim3(256), 0,
                       as_stream(stream), cap, words(log_mask), words(log_speed), words(log_cols), log_n, idx, idx_n, idx_cap,
                       words(out_mask), words(out_speed), words(out_cols));
    AV_LAUNCH_CHECK();
    return AV_OK;
}
