// H: one TIME-STEP of the hot loop for every stream in ONE launch (BASELINE config 4: "64 concurrent synthetic streams batched
// through detector -> tracker -> KF -> planner, hipGraph-captured per-step"; the reference's per-frame cadence, demo.py:97-120).
//
// With one frame per stream and launch the four stage kernels are latency chains of a few microseconds each, and a step is
// their launches: four graph nodes, ~60 us per step of 64 frames, of which ~16 us graph replay and 23 us a planner kernel for 64
// start states.  Here the step is one kernel with role-split workgroups, every role running the stage kernels' OWN device code
// (simdet_frame, tracker_body, kf_axis_chain1 + kf_axis_tail1 -- kf_axis_body's one-frame step, same expressions -- / kf_dense_stream,
// plan_block: the stages' *_dev.h headers, which this file and the stage files both include), so the results are those of the separate
// launches bit for bit (tests/test_gpu_step.py, tests/test_gpu_step_roles.py):
//   workgroups [0, S)      stream s: simulated detections of its next frame (one thread: a 232-byte table row + box arithmetic;
//                          its wave stores their output arrays at once, in front of the role's wait for the previous step), then
//                          the tracker frame on eight replica waves, started from an LDS copy of the stream's record that
//                          tracker_body reads with LDS loads (INIT_LDS), then -- optionally -- the stream's 32-byte-per-row
//                          wire table for the all-gather (exchange.hip's format), all from the same workgroup
//   workgroups [S, 2 S)    stream s: Kalman step in the first wave (axis-separable filter in two parts -- kf_axis_chain1: the record
//                          and the planner's start state, all the next step and the planner wait for; kf_axis_tail1: the rest of
//                          the frame's output, later, on a planner wave with slack; the dense filter on one lane for a stream
//                          flagged non-separable), then the 3 C candidate trajectories spread over the workgroup's sixteen, twelve
//                          or eight waves (plan_block<1, PW>, start state read from LDS), cost ranking, outputs
// The two roles of a stream never exchange data (the planner does not consume tracks).
// av_hot_step launches one such step; av_hot_step_seq / av_hot_steps_seq keep up to four consecutive steps in flight (below).
// Three workgroup shapes (hot_step_shape picks, av_hot_step_plan reports): sixteen waves (21 trajectories in two rounds, one
// workgroup per CU: serial launches and depth 2 at 64 streams), TWELVE (two rounds as well, two workgroups per CU: depth 3 and 4, the
// headline -- a launch's lifetime counts against the step rate there, and most of it is the planner's rounds) and eight (three rounds,
// two per CU: the fallback).  Twelve waves x two workgroups are six waves per SIMD, i.e. at most 80 vector registers:
// hot_step_kernel<12> is compiled for that and takes 78 with no scratch and no scalar spill (DESIGN.md section 4b has the figures and
// what it took: each role loads its arguments inside its own branch, the debug clocks carry nothing in registers, the planner's wave
// number is a scalar value).
#include "simdet_dev.h"
#include "tracker_dev.h"
#include "kf_dev.h"
#include "planner_dev.h"

namespace {

struct StepArgs {
    int S, h, w, dcap, tcap;
    av_tracker_cfg tcfg;
    av_kf_cfg kcfg;
    PlanParams pp;
    int32_t* frame_count; const SimRow* tab; const double* cdf;
    int32_t *det_n, *det_box, *det_cls; double* det_conf; int32_t* det_status;
    unsigned char* trk_state; av_track_row* snap; int32_t* snap_n; int32_t* det2trk;
    const double* z; double *kf_state, *vstate, *plan_state;
    double *wp, *cost; int32_t* order;
    uint8_t* wire; int stream0, frame0;
    int* flags; int seq, spin, fence, stage_off;      // consecutive steps overlapped (av_hot_step_seq): see seq_enter
};

constexpr int STEP_NW = 8;

// ---- consecutive time-steps overlapped --------------------------------------------------------------------------------------------
// One launch per time-step leaves the chip to ONE kernel of 2 S workgroups whose 13 us are mostly latency (launch, first loads,
// the Kalman -> arc length -> trajectories chain, the drain of the stores), and step t + 1 only starts when step t has drained.
// What step t + 1 really needs of step t is less: its tracker role the stream's tracker table, its Kalman role the stream's
// filter state -- not the planner's 4.5 MB of waypoints.  av_hot_step_seq therefore lets the caller launch step q on HIP stream
// q mod D of D = 2..4 streams (step q + D follows step q in stream order) and orders step q + 1 behind step q per stream and role
// on the device: a counter per stream and role (0 tracker, 1 Kalman) holds the number of steps whose role has finished.  A role of
// step q waits until its counter reads q and publishes q + 1 when its persistent state is written.
// Steps land on different XCDs (measured: the predecessor's role had run on another XCD in 99.98 % of 537 600 hand-overs), each
// with an L2 of its own, so the hand-over has to go through memory:
//   * an agent-scope ACQUIRE in the consumer would be buffer_inv sc1, which drops the XCD's whole L2 -- that alone takes the
//     step from 7.9 to 15 us (every table of every workgroup is then re-read from HBM), and an agent-scope RELEASE in the publisher
//     (buffer_wbl2) waits for the XCD's dirty lines, the planner's waypoints among them.  Neither is used.
//   * Instead the few bytes that cross a step boundary -- tracker: header + rows (4 160 B) and the frame counter; Kalman: 46 doubles
//     -- are WRITTEN with device-scope stores (sc1: written through to memory) and READ once, into LDS, with device-scope loads (sc1:
//     never served from the CU's L1 or from an XCD's possibly stale L2 line); the stage code runs on the LDS copy.  Nothing else a
//     role reads was written by the previous step.  The counter is stored by the wave that wrote the record (the tracker's row-keeping
//     wave, the Kalman wave) behind an explicit s_waitcnt vmcnt(0): its stores are acknowledged, i.e. visible device-wide
//     (__syncthreads() is s_waitcnt lgkmcnt(0) + s_barrier on this target and waits for no global store); the consumer's loads are
//     issued after its poll has returned the new count.  tests/test_gpu_step.py: 150 unsynchronised steps x 64 streams at depth 2, 3, 4
//     bit-identical to the serial loop; tools/soak.py: 10^6 steps.
// The per-step outputs (detections, snapshot rows, det2trk, Kalman output, waypoints, costs, order, wire table) rotate through D
// buffer sets on the host side, so steps in flight never write the same output and the Kalman counter moves on before the
// planner has run.  All launches in flight must be RESIDENT together (each may be waiting for the one before it): hot_step_shape picks
// sixteen, twelve or eight waves per workgroup from the occupancy and refuses a depth that does not fit.  Every wait is bounded: after `spin`
// polls the workgroup sets the fault word (bit 0) and leaves without running its step, the launches behind it give up at once
// (HotLoop.synchronize raises) -- no launch can hang on a lost predecessor.
// seq_flags layout (AV_STEP_FLAG_INTS): one 128-byte line per counter -- 2 S pollers hammer them -- then the fault word's line, then
// the streams' detector frame counts at reset (the count before step q is base + q: the detections do not have to wait)
__device__ __host__ inline int flag_fault(int S) { return 64 * S; }
__device__ __host__ inline int flag_base(int S) { return 64 * S + 32; }
// 32 u64 of phase clocks (AVHOT_STEP_FENCE=8, tools/steptime.py), at an even word: 64-bit atomics need their 8-byte alignment
__device__ __host__ constexpr int flag_stats(int S) { return 65 * S + (S & 1) + 32; }
static_assert(flag_stats(1) % 2 == 0 && flag_stats(3) % 2 == 0 && flag_stats(64) % 2 == 0 && flag_stats(1) + 64 == AV_STEP_FLAG_INTS(1) &&
                  flag_stats(3) + 64 == AV_STEP_FLAG_INTS(3) && flag_stats(64) + 64 == AV_STEP_FLAG_INTS(64),
              "the phase clocks are the last 64 words of AV_STEP_FLAG_INTS and start at an even word");
// Nothing of it is carried in registers: the last stamp is kept in LDS, and whether the clocks are on and where they add up is worked
// out again at every mark.  Carried, they were live from a role's first line to its last, switched on or not -- the stamp in two
// vector registers of every wave, the switched-on lanes and the address in two scalar pairs -- which is what hot_step_kernel<12>
// was short of.
struct StepClock {                    // debug only: 100-MHz clock stamps of a role's thread 0, summed per phase over all launches
    const StepArgs& a;
    int role;
    unsigned long long* t;            // in LDS
    __device__ __forceinline__ bool on() const {
        int fence = a.fence;
        asm volatile("" : "+s"(fence));           // (a value of its own at every mark, or the compiler keeps the first one's lane mask)
        return (fence & 8) && a.flags && threadIdx.x == 0;
    }
    __device__ __forceinline__ unsigned long long* acc() const {
        return reinterpret_cast<unsigned long long*>(a.flags + flag_stats(a.S)) + role * 16;
    }
    __device__ __forceinline__ void start() {
        if (!on()) return;
        *t = __builtin_amdgcn_s_memrealtime();
        atomicAdd(acc() + 15, 1ull);
    }
    __device__ __forceinline__ void mark(int k) {
        if (!on()) return;
        const unsigned long long n = __builtin_amdgcn_s_memrealtime();
        atomicAdd(acc() + k, n - *t);
        *t = n;
    }
};

// The poll of one role of one stream, by ONE thread: true when the predecessor's counter has reached this step's number, false
// (fault word set) when the wait ran out or another wait had.
__device__ __forceinline__ int seq_poll(const StepArgs& a, int slot) {
    int ok = 0;
    // (locals: with the arguments read through `a` inside the loop the compiler reloads them from the kernel-argument segment on
    // every poll, a scalar-cache round trip in front of each device-scope load)
    int* const counter = a.flags + 32 * slot;
    int* const fault = a.flags + flag_fault(a.S);
    const int want = a.seq, spin = a.spin;
    for (int n = 0; n <= spin; ++n) {
        // (step numbers are 32-bit and wrap -- three hours of stepping at this rate -- so "has reached" is a signed distance)
        if ((int)((unsigned)__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - (unsigned)want) >= 0) { ok = 1; break; }
        // (once any wait has run out the chain is broken for good: the launches behind it give up at once instead of one timeout each)
        if ((n & 255) == 255 && __hip_atomic_load(fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
    }
    if (!ok) atomicOr(a.flags + flag_fault(a.S), 1);
    if (ok && (a.fence & 8) && a.seq != 0) {      // debug: publisher's clock at its counter store -> this poll's return
        const unsigned long long tp = __hip_atomic_load(reinterpret_cast<unsigned long long*>(a.flags + 32 * slot + 2), __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        unsigned long long* acc = reinterpret_cast<unsigned long long*>(a.flags + flag_stats(a.S)) + (slot & 1) * 16;
        if (now > tp) atomicAdd(acc + 8, now - tp), atomicAdd(acc + 9, 1ull);
    }
    return ok;
}
// The tracker role's wait: thread 0 polls, the waves that fetch the record are others, so all of them meet at a workgroup barrier
// between the poll and their loads.
__device__ __forceinline__ bool seq_enter(const StepArgs& a, int slot, int* go) {
    if (threadIdx.x == 0) *go = seq_poll(a, slot);
    __syncthreads();                  // (also keeps the compiler from moving any load of the role above the poll)
    if (!*go) return false;
    if (a.fence & 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // debug: the form the comment above prices
    return true;
}
// by ONE thread, behind a workgroup barrier that follows the role's last (device-scope) store to its persistent state
__device__ __forceinline__ void seq_leave(const StepArgs& a, int slot) {
    if (a.fence & 2) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (a.fence & 8)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(a.flags + 32 * slot + 2), __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.flags + 32 * slot, (int)((unsigned)a.seq + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The persistent records as the roles address them: explicitly in the global address space.  A pointer that has been pinned in
// registers (below) no longer tells the compiler where it points, and a load or store through it would be a flat_ instruction; the
// hand-over's loads and stores are global_ ones.
typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) int32_t gi32;

// n8 8-byte words of a stream's record into LDS, by the `nthreads` threads of the workgroup from thread `first` on, at most two words
// per thread (n8 <= 2 nthreads: hot_step_prepare admits tcap 64 only).  Both loads of a thread are issued before its first wait --
// one round trip to memory, not two -- hence straight-line code, no loop, and the kind of load a template argument, not a branch
// beside each load.  COHERENT: device-scope loads (the record was written by the previous step, possibly on another XCD).
template <bool COHERENT>
__device__ __forceinline__ void fetch_record(gu64* g, void* dst_lds, int n8, int first, int nthreads) {
    unsigned long long* l = reinterpret_cast<unsigned long long*>(dst_lds);
    const int i = (int)threadIdx.x - first, j = i + nthreads;
    if (i < 0 || i >= nthreads) return;
    const bool p0 = i < n8, p1 = j < n8;
    unsigned long long v0 = 0, v1 = 0;
    if (p0) v0 = COHERENT ? __hip_atomic_load(g + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : g[i];
    if (p1) v1 = COHERENT ? __hip_atomic_load(g + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : g[j];
    if (p0) l[i] = v0;
    if (p1) l[j] = v1;
}
static_assert((HDR_INTS * 4 + 64 * (int)sizeof(av_track_row)) / 8 <= 2 * (STEP_NW * 64 - 64) && AV_KF_STATE_DOUBLES <= 64,
              "fetch_record: two words per thread cover the tracker's record (tcap 64), one the filter's");

// The kernel's arguments as a ROLE reads them: from the kernel-argument segment (StepArgs is the kernel's only parameter, at its
// offset 0), through a pointer the compiler cannot trace back to the parameter.  Read from the parameter, all ~130 scalar registers
// of arguments -- both roles' -- are loaded at the kernel's entry and most of them spilled to vector-register lanes at once (148-152
// of them, three vector registers); read through this, a role's loads are scalar loads placed inside its own branch, and only its own.
__device__ __forceinline__ const StepArgs& role_args() {
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const StepArgs*)p;
}

// PW: waves of a planner workgroup (the tracker role always runs on STEP_NW = 8; with PW = 16 or 12 its workgroups' other waves leave
// at once).  The 3 C = 21 trajectories of a start state are dealt to the waves whole: eight waves take three rounds, twelve and
// sixteen two (twelve: the three phase-1 pair waves one trajectory each, the nine others two).
template <int PW>
__device__ __forceinline__ void hot_step_body(const StepArgs& a0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int go, fc_stage;
    __shared__ unsigned long long ck_t;
    __shared__ __attribute__((aligned(16))) double kf_stage[AV_KF_STATE_DOUBLES + 2];
    // the Kalman wave's hand-off inside the workgroup: the planner's start state (px, py, heading, speed), what the tail of the
    // Kalman step needs beside the record, and whether there is a tail to run (the dense filter does everything at once)
    __shared__ __attribute__((aligned(32))) double kf_start[4];
    __shared__ __attribute__((aligned(16))) double kf_carry[KF_CARRY_DOUBLES];
    __shared__ int kf_tail;
    // the step's inputs that do not come from the previous step, in LDS before the wait: the frame's detections (made here, copied
    // to their output arrays by thread 0's wave, also in front of the wait) and the ego measurement
    __shared__ __attribute__((aligned(16))) int d_box[8 * 4];
    __shared__ __attribute__((aligned(16))) double d_conf[8], d_area[8], z_stage[4];
    __shared__ int d_cls[8], d_n[1];
    const int tid = threadIdx.x;
    const bool seq = a0.flags != nullptr;          // consecutive steps overlapped: wait for / publish to the neighbouring launches
    // Both roles run on an LDS copy of the stream's record (tracker: header + rows; Kalman: the filter's 46 doubles), fetched by the
    // whole workgroup at once -- with device-scope loads and stores when the neighbouring steps are separate launches in flight.
    if ((int)blockIdx.x < a0.S) {
        const StepArgs& a = role_args();
        if (PW > STEP_NW && tid >= STEP_NW * 64) return;
        const int s = blockIdx.x;
        StepClock ck{a, 0, &ck_t};
        ck.start();
        // the detections first: overlapped, the detector's count before step q is its count at reset + q -- no need to wait for step
        // q - 1 (tid 0 checks that against the counter the predecessor left: fault bit 1)
        int fc_before = 0;
        if (tid == 0) {
            fc_before = seq ? (int)((unsigned)a.flags[flag_base(a.S) + s] + (unsigned)a.seq) : a.frame_count[s];
            fc_stage = fc_before;
            simdet_frame<true>(0, 0, 0, a.h, a.w, a.dcap, &fc_stage, a.tab, a.cdf, d_n, d_box, d_cls, d_conf,
                               a.det_status ? a.det_status + s : nullptr);
            for (int i = 0; i < a.dcap; ++i)      // the boxes' areas, as the tracker's chunk hand-over makes them (exact in float64)
                d_area[i] = (double)(d_box[4 * i + 2] - d_box[4 * i]) * (double)(d_box[4 * i + 3] - d_box[4 * i + 1]);
        }
        // The detections' output arrays, by thread 0's own wave (dcap <= 8 lanes of it) and IN FRONT of the wait: the tracker reads
        // the LDS copy, the arrays serve only the caller, and this step's output set is free (sets rotate per step; the previous
        // user of the set has finished in stream order).  Stored behind the record fetch they were four unacknowledged stores of
        // column wave 0 in the middle of the chain; here their acknowledgements arrive while the role waits for its predecessor.
        if (tid < 64) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
            if (tid < a.dcap) {
                reinterpret_cast<int4*>(a.det_box)[(size_t)s * a.dcap + tid] = reinterpret_cast<const int4*>(d_box)[tid];
                a.det_cls[(size_t)s * a.dcap + tid] = d_cls[tid];
                a.det_conf[(size_t)s * a.dcap + tid] = d_conf[tid];
                if (tid == 0) a.det_n[s] = d_n[0];
            }
        }
        ck.mark(0);                   // detections made, their output arrays stored
        // What the role needs right behind its wait is worked out in front of it, and pinned there: none of it depends on the
        // predecessor, and left to the compiler the kernel-argument loads and the address arithmetic sit between the poll's barrier
        // and the first record load, on the stream's chain.
        int stage_off = a.stage_off, n8 = (HDR_INTS * 4 + a.tcap * (int)sizeof(av_track_row)) / 8;
        gu64* rec = (gu64*)(a.trk_state + (size_t)s * state_bytes(a.tcap, a.tcfg.trajectory_length));
        gi32* fcp = (gi32*)(a.frame_count + s);
        asm volatile("" : "+s"(stage_off), "+s"(n8), "+s"(rec), "+s"(fcp));
        if (seq && !seq_enter(a, 2 * s, &go)) return;
        ck.mark(1);                   // waited for the predecessor
        unsigned char* stage = smem + stage_off;
        int fc0 = 0;
        if (seq && tid == 0) fc0 = __hip_atomic_load(fcp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (in flight with the table)
        // (by the waves thread 0 is not in: launched serially, the record comes in while thread 0 still makes the detections)
        if (seq)
            fetch_record<true>(rec, stage, n8, 64, STEP_NW * 64 - 64);
        else
            fetch_record<false>(rec, stage, n8, 64, STEP_NW * 64 - 64);
        if (tid == 0) {
            if (seq) {
                if (fc0 != fc_before) atomicOr(a.flags + flag_fault(a.S), 2);
                __hip_atomic_store(fcp, fc_stage, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                *fcp = fc_stage;
            }
        }
        if (seq) __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): thread 0's frame-counter store is acknowledged before any wave passes the barrier
        __syncthreads();              // the detections and the table copy are in LDS
        ck.mark(2);                   // record in LDS
        // (INIT_LDS: the staged record is read with LDS loads -- no flat load, no vmcnt wait between this barrier and the first exchange)
        tracker_body<false, 8, STEP_NW, 0, true>(a.tcfg, 1, a.dcap, d_n, d_box, d_cls, d_conf, a.tcap, a.trk_state, a.snap, a.snap_n,
                                                 a.det2trk, 1, s, smem, 0xFEDCBA9876543210ull, stage, seq, 0,
                                                 seq ? a.flags + 32 * (2 * s) : nullptr, (int)((unsigned)a.seq + 1u), (a.fence & 8) != 0,
                                                 d_area);
        // (overlapped: the wave that keeps the complete rows has published the step counter itself, behind an s_waitcnt vmcnt(0) on its
        // record stores -- __syncthreads() compiles to s_waitcnt lgkmcnt(0) + s_barrier on this target and waits for no global store --
        // and written the snapshot rows after that; the successor may start before the wire table is written: the steps in flight have
        // wire buffers of their own)
        ck.mark(3);                   // tracker frame (thread 0's wave)
        if (a.wire) {                 // this stream's table in wire format (pack_tracks_kernel's row conversion)
            __syncthreads();          // the snapshot rows the bookkeeper wave wrote
            // frame = frame0 + the stream's detector frame count after this step (a captured graph -- fixed kernel arguments -- stamps
            // every replay with its own index)
            if (tid < a.tcap)
                wire_put(a.wire + (size_t)s * (AV_WIRE_HDR_BYTES + (size_t)a.tcap * AV_WIRE_ROW_BYTES), tid, a.snap_n[s], a.tcap,
                         a.snap + (size_t)s * a.tcap, a.stream0 + s, a.frame0 + fc_stage);
        }
    } else {
        const StepArgs& a = role_args();
        const int s = blockIdx.x - a.S;
        size_t s64 = (size_t)s;       // (pinned as a scalar value: the compiler otherwise widens s inside the branch below, per lane)
        asm volatile("" : "+s"(s64));
        StepClock ck{a, 1, &ck_t};
        ck.start();
        if (tid < 4) z_stage[tid] = a.z[s64 * 4 + tid];
        // The Kalman wave does only what the NEXT STEP waits for before it publishes (kf_axis_chain1: the record and the planner's
        // start state, left in LDS); the rest of the frame's Kalman output (kf_axis_tail1) is made later by a planner wave with slack.
        // What it needs behind its wait -- addresses and filter settings, none of which the predecessor writes -- is in registers
        // before it (pinned: the compiler otherwise loads them from the kernel-argument segment behind the poll, on the chain).
        // (the arrays' bases, not the stream's addresses: the compiler adds a shifted index on the vector unit, which does not pin)
        gu64* rec = (gu64*)a.kf_state;
        long long kbits[3];           // (the settings as bit patterns: a double does not pin to scalar registers either)
        static_assert(sizeof(kbits) == sizeof(av_kf_cfg), "av_kf_cfg is three doubles");
        __builtin_memcpy(kbits, &a.kcfg, sizeof(kbits));
        asm volatile("" : "+s"(rec), "+s"(kbits[0]), "+s"(kbits[1]), "+s"(kbits[2]));
        rec += s64 * AV_KF_STATE_DOUBLES;
        // (the output addresses are worked out where they are used, on the rare dense path and in the tail: kept from here they are
        // four more registers through the chain, which has none to spare)
        auto vs = [&] { return a.vstate + s64 * AV_VSTATE_DOUBLES; };
        auto ps = [&] { return a.plan_state + s64 * 4; };
        av_kf_cfg kc;
        __builtin_memcpy(&kc, kbits, sizeof(kc));
        // The wave that polls is the wave that fetches the record: it goes from its matched poll straight to its loads, without a
        // workgroup barrier in between (the wavefront-scope fence is no instruction; it keeps the compiler from moving the loads up).
        // The other waves learn `go` at the barrier that releases the planner.
        if (tid < 64) {
            int ok = 1;
            if (seq) {
                if (tid == 0) go = ok = seq_poll(a, 2 * s + 1);
                ok = __builtin_amdgcn_readfirstlane(ok);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (ok && (a.fence & 1)) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // debug, as in seq_enter
            }
            if (ok) {
                ck.mark(1);
                if (seq)
                    fetch_record<true>(rec, kf_stage, AV_KF_STATE_DOUBLES, 0, 64);
                else
                    fetch_record<false>(rec, kf_stage, AV_KF_STATE_DOUBLES, 0, 64);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
                ck.mark(2);
                const bool separable = kf_axis_chain1(kc, z_stage, kf_stage, kf_start, kf_carry, tid);
                if (tid == 0) {
                    kf_tail = separable;
                    if (!separable) {     // (LDS form: kf_dense.inc; its plan_state goes to LDS for the planner and from there to its output)
                        kf_dense_stream_lds(kc, 0, 1, z_stage, nullptr, kf_stage, vs(), kf_start);
                        *reinterpret_cast<double4*>(ps()) = *reinterpret_cast<const double4*>(kf_start);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
                if (tid < AV_KF_STATE_DOUBLES) {
                    if (seq)
                        __hip_atomic_store(rec + tid, (unsigned long long)__double_as_longlong(kf_stage[tid]), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    else
                        rec[tid] = (unsigned long long)__double_as_longlong(kf_stage[tid]);
                }
            }
        }
        ck.mark(3);                   // Kalman chain + record stores issued
        __syncthreads();              // releases the planner: its start state is in LDS (no wait for any global store)
        if (seq && !go) return;       // the wait ran out: the whole workgroup leaves without its step (the Kalman wave ran none of it)
        ck.mark(4);                   // planner start
        // The Kalman wave publishes its counter itself, behind the acknowledgement of its record stores -- while the planner's phase 1
        // runs on other waves: plan_block deals its tasks from wave KF_ROT on, which leaves wave 0 without phase-1 work (it joins the
        // phase-1 barrier when its counter is stored and takes its trajectories after it: three with eight waves, two with twelve)
        constexpr int KF_ROT = 4;
        static_assert(KF_ROT + 3 < PW, "wave 0 must not be a phase-1 pair wave nor the heading wave (task wave PW - 1)");
        if (seq && tid < 64) {
            __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0)
            if (tid == 0) seq_leave(a, 2 * s + 1);
        }
        ck.mark(5);                   // record acknowledged, counter stored
        const bool clocks = seq && (a.fence & 8);
        auto tail = [&](int task_wave) {          // by the first pair wave, behind its cost chain
            if (task_wave != 0 || !kf_tail) return;
            const unsigned long long t0 = clocks ? __builtin_amdgcn_s_memrealtime() : 0ull;
            kf_axis_tail1(a.kcfg, kf_stage, kf_carry, vs(), ps(), tid & 63);
            if (clocks && (tid & 63) == 0)
                atomicAdd(reinterpret_cast<unsigned long long*>(a.flags + flag_stats(a.S)) + 16 + 7, __builtin_amdgcn_s_memrealtime() - t0);
        };
        plan_block<1, PW>(a.pp, s, a.S, kf_start, nullptr, 0, nullptr, 0, a.wp, a.cost, a.order, reinterpret_cast<double*>(smem), 0, KF_ROT,
                          tail);
        ck.mark(6);                   // planner (thread 0's wave)
    }
}

// StepArgs is, and has to stay, the ONLY parameter of these kernels: role_args() reads it at offset 0 of the kernel-argument segment.
// Anything a step needs beside it goes into StepArgs.
template <int PW>
__global__ void __launch_bounds__(PW * 64) hot_step_kernel(StepArgs a) {
    hot_step_body<PW>(a);
}
// twelve waves, two workgroups per CU: six waves per SIMD, which the register allocator is told here (<= 80 vector registers)
template <>
__global__ void __launch_bounds__(12 * 64) __attribute__((amdgpu_waves_per_eu(6))) hot_step_kernel<12>(StepArgs a) {
    hot_step_body<12>(a);
}

}  // namespace

// dynamic LDS of the tracker role: the tracker's layout for one staged frame on eight replica waves (tracker_lds_bytes), then the copy
// of the stream's header and rows the tracker role runs on, from byte stage_off on
static size_t hot_step_tracker_lds(int dcap, int tcap, int& stage_off) {
    static_assert(STEP_NW == 8, "tracker_lds_bytes sizes the replica kernel's eight column waves");
    const size_t lds_t = (tracker_lds_bytes(tcap, dcap, 1, true, 0) + 15) & ~size_t(15);
    stage_off = (int)lds_t;
    return lds_t + HDR_INTS * 4 + (size_t)tcap * sizeof(av_track_row);
}

// A workgroup shape of the step kernel: waves per workgroup, the kernel (for the launch and for the attribute and occupancy queries)
// and its static __shared__ (the Kalman bodies' arrays), which counts against the same 64 KB as the dynamic LDS.
struct StepShape {
    int waves;
    const void* fn;
    size_t lds_static;
};
template <int PW>
static StepShape hot_step_shape_of() {
    const void* fn = reinterpret_cast<const void*>(hot_step_kernel<PW>);
    hipFuncAttributes fa{};
    return {PW, fn, hipFuncGetAttributes(&fa, fn) == hipSuccess ? (size_t)fa.sharedSizeBytes : (size_t)16384};
}
// a launch as hot_step_shape decided it: the shape, the dynamic LDS (the larger of the tracker role's and the planner's), where in
// it the tracker role's copy of the stream's table starts, and the occupancy answer for that shape (0 where it was not asked: depth 1)
struct StepPlan {
    const StepShape* shape;
    size_t lds;
    int stage_off, per_cu;
};

// AV_EINVAL where no shape fits
static int hot_step_shape(const av_ctx* ctx, int n_streams, int dcap, int tcap, int depth, StepPlan& plan) {
    // Waves per workgroup: sixteen (the planner's 21 trajectories in two rounds, one workgroup per CU), else twelve (two rounds as
    // well -- the three phase-1 pair waves take one trajectory, the nine others two -- and two workgroups per CU: hot_step_kernel<12>
    // is held to 80 registers), else eight (three rounds, two per CU).  A shape is passed over when the planner's per-wave tiles do
    // not fit the LDS with it (n > 66 at 21 candidates and sixteen waves) or when `depth` launches in flight would not all be
    // resident -- every one of them may be waiting for the one before it, so depth x 2 S workgroups must fit on the device together;
    // residency is what the occupancy query answers for that instantiation, never assumed.  AVHOT_STEP_PW=8|12|16 forces one.
    static const StepShape shapes[3] = {hot_step_shape_of<16>(), hot_step_shape_of<12>(), hot_step_shape_of<8>()};      // (queried once)
    int stage_off = 0;
    const size_t lds_t = hot_step_tracker_lds(dcap, tcap, stage_off);
    const char* pwe = getenv("AVHOT_STEP_PW");
    const int forced = pwe ? atoi(pwe) : 0;
    // (left by return; a shape that does not fit falls to the next one unless it was forced)
    for (const StepShape* sh = shapes + (forced == 8 ? 2 : forced == 12 ? 1 : 0);; ++sh) {
        const size_t lds_p = plan_lds_doubles(1, ctx->n_points, ctx->n_cand, sh->waves) * 8;
        const size_t lds = lds_t > lds_p ? lds_t : lds_p;
        int per_cu = 0;
        if (lds + sh->lds_static > 64 * 1024) {
            AV_REQUIRE(sh->waves > 8 && !pwe, AV_EINVAL,
                       "av_hot_step: configuration needs %zu B of dynamic + %zu B of static LDS (limit 65536)", lds, sh->lds_static);
            continue;
        }
        if (depth > 1) {
            AV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sh->fn, sh->waves * 64, lds));
            if ((long long)depth * 2 * n_streams > (long long)per_cu * ctx->n_cus) {
                AV_REQUIRE(sh->waves > 8 && !pwe, AV_EINVAL,
                           "av_hot_step: %d launches of %d workgroups in flight do not fit the device (%d per CU x %d CUs)", depth,
                           2 * n_streams, per_cu, ctx->n_cus);
                continue;
            }
        }
        plan = StepPlan{sh, lds, stage_off, per_cu};
        return AV_OK;
    }
}

// Validates the arguments of the steps of one call -- one per buffer set, n_sets of them, all with step number seq -- fills their
// kernel arguments par[0 .. n_sets) and decides the launch they share.  z_steps: read instead of the sets' z where given.
static int hot_step_prepare(av_ctx* ctx, const av_step_loop* loop, const av_step_set* sets, int n_sets, const double* z_steps, void* wire,
                            int stream0, int frame0, int32_t* seq_flags, int seq, int depth, StepArgs* par, StepPlan& plan) {
    AV_REQUIRE(ctx && loop && sets, AV_EINVAL, "av_hot_step: null argument");
    const av_step_loop& l = *loop;
    for (int k = 0; k < n_sets; ++k) {
        const av_step_set& b = sets[k];
        AV_REQUIRE(l.frame_count && b.det_n && b.det_box && b.det_cls && b.det_conf && l.tracker_state && (z_steps || b.z) && l.kf_state &&
                       b.vstate && b.plan_state && b.cost && b.order,
                   AV_EINVAL, "av_hot_step: null argument");
    }
    AV_REQUIRE(l.n_streams > 0, AV_EINVAL, "av_hot_step: n_streams must be > 0");
    AV_REQUIRE(ctx->planner_ready && ctx->d_simtab, AV_ESTATE, "av_hot_step: call av_planner_configure first");
    for (int k = 0; k < n_sets; ++k) {
        AV_REQUIRE((sets[k].snap == nullptr) == (sets[k].snap_n == nullptr), AV_EINVAL, "av_hot_step: snap and snap_n go together");
        AV_REQUIRE(!wire || sets[k].snap, AV_EINVAL, "av_hot_step: the wire tables are made from the snapshot rows");
    }
    // the shapes the one-launch step is built for; anything else keeps the four stage calls
    AV_REQUIRE(l.tcap == 64 && l.dcap >= 7 && l.dcap <= 8 && l.tracker_cfg.iou_threshold > 0.0 && l.tracker_cfg.trajectory_length >= 1,
               AV_EINVAL, "av_hot_step: needs tcap 64, dcap 7..8 and iou_threshold > 0 (use the stage calls otherwise)");
    AV_REQUIRE(l.h > 0 && l.w > 121, AV_EINVAL, "av_hot_step: frame %dx%d too small", l.w, l.h);
    AV_REQUIRE(((uintptr_t)seq_flags & 7) == 0, AV_EINVAL, "av_hot_step: the sequence flags must be 8-byte aligned (64-bit phase clocks in their last 64 words)");
    const int rc = hot_step_shape(ctx, l.n_streams, l.dcap, l.tcap, depth, plan);
    if (rc != AV_OK) return rc;
    StepArgs a{};
    a.S = l.n_streams, a.h = l.h, a.w = l.w, a.dcap = l.dcap, a.tcap = l.tcap;
    a.tcfg = l.tracker_cfg, a.kcfg = l.kf_cfg;
    fill_params(ctx, a.pp);
    a.frame_count = l.frame_count, a.tab = (const SimRow*)ctx->d_simtab, a.cdf = ctx->d_cdf;
    a.det_status = l.det_status, a.trk_state = (unsigned char*)l.tracker_state, a.kf_state = l.kf_state;
    a.wire = (uint8_t*)wire, a.stream0 = stream0, a.frame0 = frame0;
    a.flags = seq_flags, a.seq = seq;
    const char* spe = seq_flags ? getenv("AVHOT_STEP_SPIN") : nullptr;
    a.spin = spe ? atoi(spe) : (1 << 22);
    const char* fe = seq_flags ? getenv("AVHOT_STEP_FENCE") : nullptr;
    a.fence = fe ? atoi(fe) : 0;     // (debug: 1 = full agent-scope acquire in every role, the form the comment above prices)
    a.stage_off = plan.stage_off;
    for (int k = 0; k < n_sets; ++k) {
        const av_step_set& b = sets[k];
        a.det_n = b.det_n, a.det_box = b.det_box, a.det_cls = b.det_cls, a.det_conf = b.det_conf;
        a.snap = b.snap, a.snap_n = b.snap_n, a.det2trk = b.det2trk;
        a.z = z_steps ? z_steps : b.z, a.vstate = b.vstate, a.plan_state = b.plan_state;
        a.wp = b.waypoints, a.cost = b.cost, a.order = b.order;
        par[k] = a;
    }
    return AV_OK;
}

static int hot_step_go(const StepArgs& a, const StepPlan& p, av_stream_t stream) {
    void* args[] = {const_cast<StepArgs*>(&a)};
    AV_HIP(hipLaunchKernel(p.shape->fn, dim3(2 * a.S), dim3(p.shape->waves * 64), args, p.lds, as_stream(stream)));
    return AV_OK;
}

extern "C" int av_hot_step_plan(av_ctx* ctx, int n_streams, int dcap, int tcap, int depth, int* waves, int* per_cu, size_t* lds_bytes) {
    AV_REQUIRE(ctx && n_streams > 0 && depth >= 1, AV_EINVAL, "av_hot_step_plan: bad argument");
    AV_REQUIRE(ctx->planner_ready, AV_ESTATE, "av_hot_step_plan: call av_planner_configure first");
    AV_REQUIRE(tcap == 64 && dcap >= 7 && dcap <= 8, AV_EINVAL, "av_hot_step_plan: needs tcap 64, dcap 7..8");
    AV_HIP(hipSetDevice(ctx->device));
    StepPlan p;
    const int rc = hot_step_shape(ctx, n_streams, dcap, tcap, depth, p);
    if (rc != AV_OK) return rc;
    if (waves) *waves = p.shape->waves;
    if (per_cu) *per_cu = p.per_cu;
    if (lds_bytes) *lds_bytes = p.lds;
    return AV_OK;
}

extern "C" int av_hot_step_fits(av_ctx* ctx, int n_streams, int dcap, int tcap, int depth) {
    return av_hot_step_plan(ctx, n_streams, dcap, tcap, depth, nullptr, nullptr, nullptr);
}

static_assert(sizeof(av_step_set) == 104 && sizeof(av_step_loop) == 104, "av_step_set / av_step_loop: the layouts the bindings mirror");

extern "C" int av_hot_step(av_ctx* ctx, av_stream_t stream, const av_step_loop* loop, const av_step_set* set, void* wire, int stream0,
                           int frame0) {
    StepArgs a;
    StepPlan p;
    const int rc = hot_step_prepare(ctx, loop, set, 1, nullptr, wire, stream0, frame0, nullptr, 0, 1, &a, p);
    return rc != AV_OK ? rc : hot_step_go(a, p, stream);
}

extern "C" int av_hot_step_seq(av_ctx* ctx, av_stream_t stream, const av_step_loop* loop, const av_step_set* set, void* wire, int stream0,
                               int frame0, int32_t* seq_flags, int seq, int depth) {
    AV_REQUIRE(seq_flags, AV_EINVAL, "av_hot_step_seq: needs the sequence flags (AV_STEP_FLAG_INTS(n_streams) int32)");
    AV_REQUIRE(depth >= 2 && depth <= AV_STEP_MAX_DEPTH, AV_EINVAL, "av_hot_step_seq: depth %d not in [2, %d]", depth, AV_STEP_MAX_DEPTH);
    StepArgs a;
    StepPlan p;
    const int rc = hot_step_prepare(ctx, loop, set, 1, nullptr, wire, stream0, frame0, seq_flags, seq, depth, &a, p);
    return rc != AV_OK ? rc : hot_step_go(a, p, stream);
}

extern "C" int av_hot_steps_seq(av_ctx* ctx, int depth, const av_stream_t* streams, const av_step_loop* loop, const av_step_set* sets,
                                const double* z_steps, void* wire_steps, int stream0, int frame0, int32_t* seq_flags, int seq0, int n_steps) {
    AV_REQUIRE(seq_flags && n_steps > 0 && sets && streams, AV_EINVAL, "av_hot_steps_seq: bad argument");
    AV_REQUIRE(depth >= 2 && depth <= AV_STEP_MAX_DEPTH, AV_EINVAL, "av_hot_steps_seq: depth %d not in [2, %d]", depth, AV_STEP_MAX_DEPTH);
    for (int k = 0; k < depth; ++k)
        for (int j = 0; j < k; ++j)
            AV_REQUIRE(streams[k] != streams[j], AV_EINVAL, "av_hot_steps_seq: the %d steps in flight need %d different HIP streams", depth, depth);
    StepArgs par[AV_STEP_MAX_DEPTH];
    StepPlan p;
    int rc = hot_step_prepare(ctx, loop, sets, depth, z_steps, wire_steps, stream0, frame0, seq_flags, seq0, depth, par, p);
    if (rc != AV_OK) return rc;
    const size_t zb = (size_t)par[0].S * 4, wb = (size_t)par[0].S * (AV_WIRE_HDR_BYTES + (size_t)par[0].tcap * AV_WIRE_ROW_BYTES);
    for (int i = 0; i < n_steps; ++i) {
        const int q = (int)((unsigned)seq0 + (unsigned)i), k = (int)((unsigned)q % (unsigned)depth);      // (32-bit step numbers wrap)
        StepArgs& a = par[k];
        a.seq = q;
        if (z_steps) a.z = z_steps + (size_t)i * zb;
        if (wire_steps) a.wire = (uint8_t*)wire_steps + (size_t)i * wb;
        if ((rc = hot_step_go(a, p, streams[k])) != AV_OK) return rc;
    }
    return AV_OK;
}
