// libtarokenv: HIP kernels + C ABI (include/tarok_env.h).  gfx950 only.
//
// One thread per game, 256-thread workgroups (4 waves).  Per-game state is the
// 4 packed uint64 lanes of tarok_device.h, stored as two 16-byte SoA arrays
// (s01[g] = play pair {X0,X1}, s23[g] = seat pair {Y0,Y1}): every wave-level
// load/store moves 1 KiB contiguous.  The work is integer mask algebra + popcounts (no MFMA): the
// one-card step (k_step: the state through HBM on every card) is bounded by HBM bandwidth once the batch
// streams, the multi-card Bot-policy kernel (k_play_wide: the state stays in registers) by instruction issue.
//
// Finished games are replaced at once (auto-reset) without a deal on the step's critical path:
// every slot keeps its next FOURTEEN games ready in the lines of its Aux record (episode e lives in
// line e mod 14).  A launch that consumes episode k pushes "deal k+14 into line k mod 14" onto its
// workgroup's refill list; the NEXT launch carries extra workgroups that work those lists off
// (sorting-network deals on dense lanes) while its own play workgroups run — the ~5 us of deal
// latency overlaps the next launch instead of following this one.  The shortest game, a Berac lost on
// trick 1, is 4 cards: with fourteen lines launches of 128 cards (32 tricks; a slot starts ~3.5 games
// in one) practically never wait for a deal (with seven, round 1, 64 cards were the limit: a slot that
// finishes more games within two launches than it has lines deals in place, and the launch is its
// slowest wave).  Lists are double-buffered by launch parity — the low bit of the launch number, which is kept
// modulo 64 in DEVICE memory as counts of started workgroups that every step launch advances by its grid size
// (launch_count / launch_counted / launch_phase; two kinds of launch with two grid sizes, each counted on its own,
// the launch number is the sum), so eager launches and replays of captured graphs (the library's own or a caller's,
// e.g. torch.cuda.graph) mix freely and in any number.  The one-card step of small batches (kind 0) has no extra
// workgroups: every step workgroup works its own group's lists off after playing its card, and it does not deal the
// lines it empties in the next launch at all but collects them for a bulk deal every thirty-second launch
// (refill_role<true>, TAROK_OPT_LAZY_REFILL).  A line is valid iff its episode tag matches
// and it is not being re-dealt right now (`cprev` in the slot's state), and a slot that ever runs
// out of usable lines just deals the game itself, wave-cooperatively (ballot/readlane), same result.
#include "tarok_device.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tuple>
#include <type_traits>
#include <utility>

#include "../../include/tarok_env.h"

#define TK_BLOCK 256               // game slots per play workgroup (the MLP and learner kernels are laid out for 256)
#define TK_PF_SLOTS (4 * TK_BLOCK)
#define TK_GRAPH_CACHE 16          // instantiated graphs kept per env (tarok_run_random)
#define TK_REFILL_CAP (TK_BLOCK * TK_AHEAD) // refill-list entries per play workgroup and launch (<= TK_AHEAD per slot)
#define TK_REFILL_FAN 8            // play workgroups whose lists one refill workgroup works off
// list lengths: one 128-byte line per (play workgroup, parity) — neighbouring workgroups run on
// different XCDs, whose L2s are not coherent: two of them must never write into one line
#define TK_RC(group, k) ((((size_t)(group)) * 4 + (k)) * 32)     // k = 0, 1: the per-launch lists by parity; 2, 3: the one-card step's stretch lists
#define TK_BULK_EVERY 32u          // one-card launches per stretch (a power of two; see launch_count): the stretch lists are dealt in bulk this often
#define TK_BULK_CAP ((TK_BULK_EVERY / 4) * TK_BLOCK)  // entries of a stretch list: a game is at least four cards long, one card per launch

#define TK_AHEAD TAROK_GAMES_AHEAD  // next-game lines per slot (<= 15: epar and cprev are 4 bits each)
#define TK_LINE(episode) ((u32)(episode) % (u32)TK_AHEAD)
#define TK_FINQ 128                 // entries of a play wave's finished-games ring (a power of two >= 128)
// The per-card outputs are written once and never read back by the kernels: non-temporal stores, so that
// they stream out during the launch instead of piling up as dirty L2 lines for the write-back at its end
#define TK_STREAM_STORE(ptr, val) __builtin_nontemporal_store((val), (ptr))
// s_waitcnt vmcnt(0) (gfx9 encoding: expcnt and lgkmcnt left at their maxima)
#define TK_WAIT_LOADS() __builtin_amdgcn_s_waitcnt(0x0F70)
// wave-uniform branches of the card loop (play_role): a taken branch costs a lone wave ~25 cycles, one that falls
// through ~7 (tools/valu_issue: br_taken / br_not) — the usual path is laid out as the fall-through.
#define TK_RARE(c) __builtin_expect(!!(c), 0)
#define TK_USUAL(c) __builtin_expect(!!(c), 1)

// Per-slot side record: TK_AHEAD (fourteen) 64-byte next-game lines.  Line b holds the dealt-ahead
// game whose episode number is b mod TK_AHEAD: its packed pairs, its RNG key and the episode number
// it is (the validity tag).  A 64-byte AuxLine is HALF an L2 line (128 B on MI355X), and a slot's
// 448-byte record shares its first / last L2 line with a neighbouring slot.  That is safe because
// (i) only refill workgroups ever write these records — play workgroups read them and write
// nothing here (their Counters / state / gkey / refill lists live in lines of their own, see
// Counters below), (ii) all lines of one play group's 256 slots (a 112 KiB, 128-byte aligned
// range) are re-dealt by ONE refill workgroup per launch, so no L2 line is written by two
// workgroups (two XCDs) within a launch, and (iii) a reader never trusts a line whose episode tag
// does not match or that `cprev` says is being re-dealt right now.
struct __attribute__((aligned(64))) AuxLine {
    ulonglong2 n01, n23; u64 nkey; u32 nep;
    u32 pad[5];
};
struct __attribute__((aligned(64))) Aux { AuxLine line[TK_AHEAD]; };
static_assert(sizeof(AuxLine) == 64 && sizeof(Aux) == 64 * TK_AHEAD, "64 bytes per next-game line");
static_assert((TK_BLOCK * sizeof(Aux)) % 128 == 0, "a play group's next-game lines end on an L2 line boundary");
static_assert(TK_AHEAD >= 2 && TK_AHEAD <= 15, "epar / cprev are 4-bit fields");
// What a finishing game always touches: the slot's episode number and its summed scores.  Kept
// apart from the next-game lines: those are written by refill workgroups, these by the slot's own
// play workgroup, which runs on another XCD (another, non-coherent L2) — the two must not share
// a cache line.
struct __attribute__((aligned(32))) Counters {
    int4 score_sum;                                  // summed scores by seat (Tarok.rezultati)
    u32 episode;                                     // episode number of the slot's current game
    u32 pad[3];
};
static_assert(sizeof(Counters) == 32, "Counters is half a cache line");

struct tarok_env {
    int device;
    int64_t n;
    u64 offset, seed;
    int mix, flags;
    ulonglong2 *s01, *s23;   // packed state
    Aux *aux;                // next-game lines per slot
    Counters *cnt;           // episode number and score sums per slot
    uint16_t *nstale;        // bit k: the game k+1 ahead is missing and not on any refill list
                             // (after tarok_reset; what k_prefetch scans); padded to 1024 slots
    u64 *gkey;               // RNG key of the slot's current game
    uint8_t *hist;           // [48][n] play history (card p of the slot's current game), TAROK_HISTORY envs only
    u64 *rlist;              // refill lists [play workgroups][2 parities][TK_REFILL_CAP]: episode<<32 | slot in group
    u32 *rcount;             // [play workgroups][4] list lengths, one 128-byte line each (TK_RC)
    u64 *elist;              // the one-card step's stretch lists [play workgroups][2][TK_BULK_CAP] (refill_role)
    u32 *epoch;              // 2 x TK_EPOCH_SHARDS counters, 128 bytes apart: workgroups of step launches of either kind started so
                             // far (launch_count): the parity of the refill list the running launch writes (it works the other one off)
    uint32_t refill_fan;     // play workgroups per refill workgroup (1..TK_REFILL_FAN)
    uint32_t lazy_refill;    // the one-card step lists emptied lines for a bulk deal every TK_BULK_EVERY launches (refill_role)
    int n_cus;               // compute units of the device (k_learn_dw's grid), 0 = not asked yet
    float *adam_sumsq;       // k_learn_gnorm's partial sums
    u64 *bid_deal;           // tarok_playout_bids: the deal being bid on, [5][n] (k_bid_deal); allocated by its first call
    u64 *stamps;             // diagnostics only (tarok_debug_stamps)
    size_t stamps_words;     // its capacity: a kernel that would write more gets no stamps pointer
    float temperature, epsilon;   // the play mode as given (tarok_set_play_mode); (1, 0): the MODE = 0 kernels, untouched
    float inv_t, eps_p;      // what the MODE = 1 kernels take: 1 / temperature (1 when greedy), thr / 2^24 ...
    uint32_t explore_thr;    // ... thr = floor(epsilon * 2^24) ...
    int greedy, mode_on;     // ... temperature == 0; mode_on: the mode is not (1, 0)
    int launched;            // a step launch has been issued (tarok_set_option: a change of the grid must restart the launch counters)
    hipStream_t cap_stream;  // capture-only stream for tarok_run_random's graphs
    // tarok_run_random's instantiated graphs.  An exec is NEVER destroyed while launches of it may still be queued (round 3
    // destroyed the one cached exec whenever the segment kind changed, with up to a hundred of its launches in flight):
    // every (launch kind, chunk, flags, buffers, launch tuning) keeps its exec until tarok_destroy, which synchronises the
    // device first; a full cache is emptied behind a device synchronisation.
    struct GraphEntry {
        hipGraphExec_t exec;
        int fused, chunk, flags, prefetch;
        void *action, *reward, *done, *obs, *stamps;
        uint32_t fan, lazy;
    } graphs[TK_GRAPH_CACHE];
    int n_graphs;
};

static thread_local int g_last_hip = 0;

#define HIPCHK(x)                                                   \
    do {                                                            \
        hipError_t e_ = (x);                                        \
        if (e_ != hipSuccess) { g_last_hip = (int)e_; return TAROK_EHIP; } \
    } while (0)

static inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + TK_BLOCK - 1) / TK_BLOCK)); }

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
__device__ __forceinline__ void load_game(Game &g, const ulonglong2 *s01, const ulonglong2 *s23, int64_t i) {
    ulonglong2 a = s01[i], b = s23[i];
    unpack(g, a.x, a.y, b.x, b.y);
}
// the play pair always; the seat pair only when the A/B planes (or the setup fields) changed
__device__ __forceinline__ void store_game(const Game &g, ulonglong2 *s01, ulonglong2 *s23, int64_t i,
                                           bool seats_changed = true) {
    ulonglong2 a;
    pack_play(g, a.x, a.y);
    s01[i] = a;
    if (seats_changed) {
        ulonglong2 b;
        pack_seats(g, b.x, b.y);
        s23[i] = b;
    }
}

// Igra.razdeli + engine construction + talon exchange for every slot.
TK_KERNEL(TK_BLOCK, 80) void k_reset(
    int64_t n, u64 seed, u64 offset, u32 episode, int mix, int flags,
    const uint8_t *__restrict__ deals, const int8_t *__restrict__ contract, const int8_t *__restrict__ declarer,
    const int8_t *__restrict__ king, const int8_t *__restrict__ choice, const uint8_t *__restrict__ discards,
    ulonglong2 *__restrict__ s01, ulonglong2 *__restrict__ s23, Aux *aux, Counters *__restrict__ cnt,
    uint16_t *__restrict__ nstale, u64 *__restrict__ gkey) {
    TK_VGPR_TOP(80, 79);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 key = game_key(seed, offset + (u64)i, episode);
    u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, tal = 0;
    bool bad = false;
#pragma unroll
    for (int b = 0; b < TK_AHEAD; b++) { aux[i].line[b].nep = 0xFFFFFFFFu; aux[i].line[b].pad[0] = 0; }   // all next-game lines: empty, no front mark (tarok_front_lines; episode 0 is never dealt ahead)
    nstale[i] = (uint16_t)((1u << TK_AHEAD) - 1);
    if (deals) {
        const uint8_t *p = deals + i * 54;
        u64 h[4] = {0, 0, 0, 0};
        u64 seen = 0;
        for (int k = 0; k < 48; k++) { u32 c = p[k]; bad |= c >= 54; c &= 63; seen |= 1ULL << c; h[k / 12] |= 1ULL << c; }
        for (int k = 0; k < 6; k++) { u32 c = p[48 + k]; bad |= c >= 54; c &= 63; seen |= 1ULL << c; tal |= (u64)c << (6 * k); }
        bad |= seen != TK_DECK;
        h0 = h[0]; h1 = h[1]; h2 = h[2]; h3 = h[3];
    } else {
        deal_thread(key, h0, h1, h2, h3, tal);
    }
    u32 c, d, k;
    if (contract) {
        int ci = contract[i];
        bad |= ci < 0 || ci > 9;
        c = (u32)ci % 10u;
        d = declarer ? ((u32)declarer[i] & 3u) : 0u;
        k = king ? ((u32)king[i] & 3u) : 0u;
    } else {
        sample_setup(key, mix, c, d, k);
    }
    Game g;
    setup_game(g, h0, h1, h2, h3, tal, c, d, k);
    g.epar = TK_LINE(episode); g.cprev = 0;
    if (g.phase == TK_PHASE_EXCHANGE && !(flags & TAROK_DEFER_EXCHANGE)) {
        if (choice && discards) {
            const uint8_t *q = discards + i * 3;
            apply_exchange(g, (u32)(uint8_t)choice[i], q[0], q[1], q[2]);
        } else {
            bot_exchange(g, key);
        }
    }
    if (bad) g.error = 1;
    store_game(g, s01, s23, i);
    gkey[i] = key;
    cnt[i].episode = episode;
    if (flags & TAROK_CLEAR_COUNTERS) cnt[i].score_sum = make_int4(0, 0, 0, 0);
}

// Deal game `episode` of slot j ahead of time into its line (episode mod TK_AHEAD).
__device__ __forceinline__ void deal_into_buffer(Aux *aux, int64_t j, u32 episode, u64 seed, u64 offset, int mix) {
    u64 key = game_key(seed, offset + (u64)j, (u64)episode);
    u64 h0, h1, h2, h3, tal;
    deal_thread(key, h0, h1, h2, h3, tal);
    u32 c, d, k;
    sample_setup(key, mix, c, d, k);
    Game g;
    setup_game(g, h0, h1, h2, h3, tal, c, d, k);
    g.epar = TK_LINE(episode); g.cprev = 0;
    if (g.phase == TK_PHASE_EXCHANGE) bot_exchange(g, key);
    ulonglong2 a, b;
    pack(g, a.x, a.y, b.x, b.y);
    AuxLine *ln = &aux[j].line[TK_LINE(episode)];
    ln->n01 = a; ln->n23 = b; ln->nkey = key; ln->nep = episode;
}

// tarok_prefetch: fill, synchronously, the next-game lines that tarok_reset emptied (flags in
// nstale: bit k = episode+1+k missing).  Each workgroup compacts the missing lines of its
// 1024-slot tile into an LDS list (4 flag bytes per thread) and deals list entry j on thread j,
// so the sorting network runs on dense lanes.
TK_KERNEL(TK_BLOCK, 128) void k_prefetch(int64_t n, u64 seed, u64 offset, int mix,
                                                      Aux *aux, const Counters *__restrict__ cnt,
                                                      uint16_t *__restrict__ nstale) {
    TK_VGPR_TOP(128, 127);
    __shared__ unsigned short list[TK_AHEAD * TK_PF_SLOTS];
    __shared__ u32 count;
    int64_t base = (int64_t)blockIdx.x * TK_PF_SLOTS;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    const u64 ALL = (1u << TK_AHEAD) - 1;
    u64 f = reinterpret_cast<const u64 *>(nstale + base)[threadIdx.x];   // 4 slots x 16 flag bits; the array is padded
    if (f) {
        u32 c = (u32)__popcll(f & (0x0001000100010001ULL * ALL));
        u32 pos = atomicAdd(&count, c);
#pragma unroll
        for (u32 k = 0; k < 4; k++) {
            u32 fk = (u32)(f >> (16 * k)) & (u32)ALL;
#pragma unroll
            for (u32 b = 0; b < TK_AHEAD; b++)
                if (fk & (1u << b)) list[pos++] = (unsigned short)((threadIdx.x * 4 + k) * TK_AHEAD + b);
        }
        reinterpret_cast<u64 *>(nstale + base)[threadIdx.x] = 0;
    }
    __syncthreads();
    u32 total = count;
    for (u32 j = threadIdx.x; j < total; j += TK_BLOCK) {
        int64_t i = base + list[j] / TK_AHEAD;
        if (i >= n) continue;
        deal_into_buffer(aux, i, cnt[i].episode + 1 + (list[j] % TK_AHEAD), seed, offset, mix);
    }
}

TK_KERNEL(TK_BLOCK, 64) void k_exchange(int64_t n, const int8_t *__restrict__ choice,
                                                      const uint8_t *__restrict__ discards,
                                                      ulonglong2 *__restrict__ s01, ulonglong2 *__restrict__ s23,
                                                      const u64 *__restrict__ gkey) {
    TK_VGPR_TOP(64, 63);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    Game g;
    load_game(g, s01, s23, i);
    if (g.phase != TK_PHASE_EXCHANGE) return;
    if (choice && discards) {
        const uint8_t *q = discards + i * 3;
        apply_exchange(g, (u32)(uint8_t)choice[i], q[0], q[1], q[2]);
    } else {
        bot_exchange(g, gkey[i]);
    }
    store_game(g, s01, s23, i);
}

TK_KERNEL(TK_BLOCK, 64) void k_legal(int64_t n, const ulonglong2 *__restrict__ s01,
                                                   const ulonglong2 *__restrict__ s23, u64 *__restrict__ obs,
                                                   int8_t *__restrict__ seat) {
    TK_VGPR_TOP(64, 63);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    Game g;
    load_game(g, s01, s23, i);
    obs[i] = obs_word(g, false);
    if (seat) seat[i] = (int8_t)((g.leader + g.nt) & 3);
}

TK_KERNEL(TK_BLOCK, 64) void k_policy(int64_t n, const u64 *__restrict__ obs,
                                                    const u64 *__restrict__ gkey, uint8_t *__restrict__ action) {
    TK_VGPR_TOP(64, 63);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 o = obs[i], key = gkey[i];     // (the key asked for WITH the observation word, not behind it: one memory round trip)
    u64 m = o & TAROK_OBS_MASK;
    u32 a = 255;
    if (m) a = policy_action(key, (u32)(o >> TAROK_OBS_STEP_SHIFT) & 63u, m);
    action[i] = (uint8_t)a;
}

// The same for four games per thread, the form the host picks for batches that stream (launch_policy): a lane of the
// one-game kernel has 16 bytes in flight, the chip 8 MB, and at 4 M games the launch ran at the memory LATENCY
// (16.3 us for 71 MB, profiles/r03_step_durations.txt; this form 13.0 us).  A workgroup takes 1,024 consecutive games; thread t the
// pairs (2t, 2t+1) of its first and of its second half, so that every load is a contiguous 16 bytes per lane and
// every store two bytes per lane of one 128-byte line per wave.
TK_KERNEL(TK_BLOCK, 64) void k_policy_x4(int64_t n, const u64 *__restrict__ obs,
                                                       const u64 *__restrict__ gkey, uint8_t *__restrict__ action) {
    TK_VGPR_TOP(64, 63);
    int64_t base = (int64_t)blockIdx.x * (4 * TK_BLOCK);
    if (base + 4 * TK_BLOCK <= n) {
        int64_t p0 = base + 2 * threadIdx.x, p1 = p0 + 2 * TK_BLOCK;
        ulonglong2 o0 = *reinterpret_cast<const ulonglong2 *>(obs + p0), o1 = *reinterpret_cast<const ulonglong2 *>(obs + p1);
        ulonglong2 k0 = *reinterpret_cast<const ulonglong2 *>(gkey + p0), k1 = *reinterpret_cast<const ulonglong2 *>(gkey + p1);
        auto one = [](u64 o, u64 key) __attribute__((always_inline)) {
            u64 m = o & TAROK_OBS_MASK;
            return m ? policy_action(key, (u32)(o >> TAROK_OBS_STEP_SHIFT) & 63u, m) : 255u;
        };
        u32 a0 = one(o0.x, k0.x) | (one(o0.y, k0.y) << 8), a1 = one(o1.x, k1.x) | (one(o1.y, k1.y) << 8);
        *reinterpret_cast<uint16_t *>(action + p0) = (uint16_t)a0;
        *reinterpret_cast<uint16_t *>(action + p1) = (uint16_t)a1;
        return;
    }
    for (int64_t i = base + threadIdx.x; i < n; i += TK_BLOCK) {       // the last, partial workgroup
        u64 o = obs[i];
        u64 m = o & TAROK_OBS_MASK;
        u32 a = 255;
        if (m) a = policy_action(gkey[i], (u32)(o >> TAROK_OBS_STEP_SHIFT) & 63u, m);
        action[i] = (uint8_t)a;
    }
}

// WHAT WORKGROUPS HAND EACH OTHER, AND THROUGH WHICH CACHE (DESIGN.md §3 has the table).  Five buffers are written by one
// workgroup and read by another: the next-game lines (`aux`: refill role -> play / step role), the per-launch refill lists
// and their lengths (`rlist`, `rcount[0..1]`: play / step role -> refill role), the stretch lists and their lengths (`elist`,
// `rcount[2..3]`: step role -> refill role and, the lengths, back to the step role of a LATER launch) and the launch counters
// (`epoch`).  Except for `epoch` every such word is read in a LATER launch than it was written: the kernel boundary (release at
// the end of a launch, acquire at the start of the next: L2 write-back and invalidate across the XCDs, vector L1 and scalar
// cache invalidated) is the only ordering the protocol relies on, and within a launch no workgroup reads a word another one
// writes in that launch.  The code says so: none of these pointers is `__restrict__` or `const` (nothing licenses the
// compiler to keep such a word in the scalar cache or to merge its reads across a barrier), every length and list entry is
// read with an agent-scope atomic load (tk_ld: a vector load that misses the L1), and `epoch` — the one buffer read and
// written within a launch — only with agent-scope atomics.
template <class T> __device__ __forceinline__ T tk_ld(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Launch number modulo TK_PHASES (see the file header) without a host counter.  The workgroups of step launches are
// counted as they START, modulo TK_PHASES times their number G per launch: launch L begins with the count at
// (L mod TK_PHASES) * G; every workgroup reads the count together with its first loads (launch_count: nothing waits for
// it alone) and adds itself afterwards (launch_counted: a wrapping increment WITHOUT a return value, behind the read in
// the lane's program order — it completes somewhere under the card loop).  At any read at most G - 1 workgroups of the
// running launch have added themselves, so the count is still in launch L's band: phase = count / G.  The kernel boundary
// drains the adds before the next launch reads.  The count is kept in TK_EPOCH_SHARDS separate counters (one 128-byte
// line each), workgroup b using counter b mod TK_EPOCH_SHARDS with G_s = the number of such workgroups: the argument
// holds for every counter on its own, and the adds do not queue up behind each other — ONE counter took 512 same-address
// atomics per launch at 65,536 games, serialised at the memory side: +3.4 us on every launch, wherever in the kernel they
// were issued (profiles/r02_ab_launch_parity.txt).
// An env has step launches of TWO grid sizes (round 4): KIND 0, the one-card step of small batches (k_step<., true>):
// `groups` workgroups, each of which plays its group's card and then works its OWN group's refill lists off — at 65,536
// games the 256 refill workgroups of the other kind, idle in fifteen launches of sixteen, cost every launch ~0.9 us
// (profiles/r04_ab_step.txt); KIND 1, every other step launch (k_play_wide, k_policy_step, the streaming k_step):
// groups + ceil(groups / fan) workgroups, play and refill roles side by side.  Each kind counts ITS launches in its own
// set of counters as above, and a workgroup of kind k reads, beside its own counter, one counter of the other kind — at
// rest during this launch: exactly (launches of that kind mod TK_PHASES) * its shard size.  The launch number is the sum.
// The low bit of the phase is the parity of the refill list the launch writes; the one-card step also works the
// next-game lines its slots emptied off in bulk, once per TK_BULK_EVERY launches (step_role, refill_role).
#define TK_EPOCH_SHARDS 256
#define TK_EPOCH_WORDS (32 * TK_EPOCH_SHARDS)      // u32 words of one kind's counters (one 128-byte line per counter)
#define TK_PHASES (2u * TK_BULK_EVERY)
static_assert((TK_BULK_EVERY & (TK_BULK_EVERY - 1)) == 0 && TK_BULK_EVERY >= 4 && TK_BULK_EVERY + 1 <= 4 * (TK_AHEAD - 1),
              "a line is dealt at most TK_BULK_EVERY + 1 launches after it was emptied and is needed again TK_AHEAD - 1 games (four launches each, at least) after that");
struct TkCount { u32 own, other; };
__device__ __forceinline__ u32 tk_shard_size(u32 grid, u32 shard) { return (grid + TK_EPOCH_SHARDS - 1 - shard) / TK_EPOCH_SHARDS; }
// the other kind's grid, and the counter of it this workgroup reads (one that exists: kind 0's grid is the smaller one)
template <int KIND> __device__ __forceinline__ u32 tk_other_grid(u32 groups, u32 fan) { return KIND == 0 ? groups + (groups + fan - 1) / fan : groups; }
template <int KIND> __device__ __forceinline__ u32 tk_other_shard(u32 groups) { return (KIND == 0 ? blockIdx.x : blockIdx.x % groups) % TK_EPOCH_SHARDS; }
template <int KIND> __device__ __forceinline__ TkCount launch_count(const u32 *epoch, u32 groups) {
    TkCount c;
    c.own = tk_ld(epoch + KIND * TK_EPOCH_WORDS + 32 * (blockIdx.x % TK_EPOCH_SHARDS));
    c.other = tk_ld(epoch + (1 - KIND) * TK_EPOCH_WORDS + 32 * tk_other_shard<KIND>(groups));
    return c;
}
// count / G_s: a float estimate (count < TK_PHASES * G_s is exact as a float for any grid a launch can have; the half added
// to the count keeps the quotient away from the integers) put right by one exact integer step either way
__device__ __forceinline__ u32 tk_div_small(u32 count, u32 g) {
    u32 q = (u32)(((float)count + 0.5f) * __builtin_amdgcn_rcpf((float)g));
    q -= (q * g > count) ? 1u : 0u;
    q += ((q + 1u) * g <= count) ? 1u : 0u;
    return q;
}
template <int KIND> __device__ __forceinline__ u32 launch_phase(TkCount c, u32 groups, u32 fan) {
    // (the counts are the same in every lane, and the compiler knows: without this fence it moves the quotients — and the wait
    // for the counts' loads — to the top of the kernel, ahead of the state loads: +4 us per launch at 4 M games)
    asm volatile("" : "+v"(c.own), "+v"(c.other));
    u32 own = tk_div_small(c.own, tk_shard_size(gridDim.x, blockIdx.x % TK_EPOCH_SHARDS));
    u32 other = tk_div_small(c.other, tk_shard_size(tk_other_grid<KIND>(groups, fan), tk_other_shard<KIND>(groups)));
    return (own + other) % TK_PHASES;
}
// call after launch_count in program order — one lane's read and add of one address stay in that order — behind a barrier
// that every wave of the workgroup passes after ITS read of the count (were this the last workgroup of its counter to add,
// a wave that read after the add would see the next launch's band), and before the first use of the count's value: the add
// counts as an outstanding memory operation of the wave, and issued only once the count has arrived it adds a memory-side
// round trip to the life of every step wave (+4 us per launch at 4 M games)
template <int KIND> __device__ __forceinline__ void launch_counted(u32 *epoch) {
    if (threadIdx.x == 0)
        (void)atomicInc(epoch + KIND * TK_EPOCH_WORDS + 32 * (blockIdx.x % TK_EPOCH_SHARDS),
                        TK_PHASES * tk_shard_size(gridDim.x, blockIdx.x % TK_EPOCH_SHARDS) - 1u);
}

// The step kernels.  One launch plays `cards` cards of every game:
//   k_step (step_role), cards = 1: tarok_step — the card comes from `action_in` (an external policy) — and
//                   tarok_step_random (the Bot policy, Igralec.py:158-159, evaluated in-kernel);
//   k_play_wide (play_role), cards >= 2, Bot policy in-kernel: cards = 4 is one whole trick = one pass of the
//                   reference's krog generator (Klop.py:47-79, Navadna_igra.py:115-141).
// The packed state is read once, stays in registers while the cards are played and is written
// once; everything a consumer of the trajectory needs is written for EVERY card: row c of
// action/obs/done/trick/reward (rows `stride` games apart) belongs to the c-th card of the launch.
// Per card: legal mask -> card -> apply -> (4th card of a trick) winner, Klop talon gift, Berac
// end, end-of-game scoring, and with TAROK_AUTO_RESET the finished game's successor swapped in
// from the slot's next-game buffer.
//
// Workgroups [0, play_groups) play; the workgroups after them work off the refill lists the
// PREVIOUS launch wrote (see the file header).
// Refill role of a step launch: work off the lists the PREVIOUS launch wrote for `fan` play
// workgroups (rblock = index among the refill workgroups; tid / nthreads = this thread in its
// workgroup), concatenated so that the sorting-network deals run on dense lanes (~11 % of the
// slots of a group finish per trick: 8 lists fill a 256-thread workgroup).  Small batches use a
// smaller fan: a refill workgroup that needs a second pass would outlast the play.
// `count` = launch_count()'s value, possibly still in flight: the list lengths of BOTH parities are requested
// before it is looked at, so the parity costs this role no memory round trip of its own.
// BULK (k_step): the lines the one-card step's slots emptied are NOT on those lists.  Every slot is at the same card of
// its trick and games end on a trick's 4th card, so they would all be dealt in the launch after it, whose refill
// workgroups (a wave alone issues an instruction every ~4.5 cycles, a deal is 2.7k of them) outlast the step
// workgroups: 9.9 us against 4.3 at 65,536 games, 79 against 44 at 4 M (profiles/r03_step_durations.txt,
// r03_ab_step.txt (e)).  A slot has fourteen lines and takes at most eight in thirty-two launches, so step_role collects
// those entries in a second pair of lists per workgroup, switched every TK_BULK_EVERY launches, and the first launch
// of each such stretch works the previous stretch's list off here, on dense lanes, in one go.  A line waits for its
// deal at most TK_BULK_EVERY launches and is not needed again before thirteen more games of its slot have
// ended (>= 52 launches); lines a slot must not meet half written — the fourteen of a slot that dealt a game in place —
// stay on the per-launch lists.  A BULK launch is of kind 0 (launch_count): it has no refill workgroups — the workgroup
// that has just played its group's card runs this role for that group alone (fan 1, rblock = its group), so the count
// has been read and counted by the step role already.  !BULK (kind 1: k_play_wide, k_policy_step, the streaming k_step;
// slots there can take a line per trick): the stretch lists of the workgroup's groups are emptied unworked — those lines
// stay stale until their slot comes round to them, deals that game in place and lists all fourteen.
template <bool BULK>
__device__ __forceinline__ void refill_role(u32 rblock, u32 tid, u32 nthreads, u64 seed, u64 offset, int mix, u32 play_groups,
                                        TkCount count, u32 *epoch, u32 fan, bool bulk_on, Aux *aux, u64 *rlist, u32 *rcount, u64 *elist) {
    constexpr int KIND = BULK ? 0 : 1;
    const u32 kind_fan = fan;            // (the env's fan: what the other kind's grid is made of)
    if (BULK) fan = 1;                   // the workgroup's own group
    u32 g0 = rblock * fan;
    // every thread loads the two per-launch lengths of every group itself, the stretch lists' lengths only in the pass that
    // works them off.  (Round 3 shipped this form because shorter ones — all four lengths with one load per wave, sums in
    // scalar registers — "failed for reasons not understood".  The reason is understood now and had nothing to do with the
    // lengths: those builds had 104 VGPRs with a shift amount of the deal in v103, and gfx950 mis-executes a 64-bit shift
    // whose amount sits in the last allocated VGPR — TK_VGPR_TOP, tarok_device.h; profiles/r04_refill_root_cause.txt.)
    u32 len0[TK_REFILL_FAN], len1[TK_REFILL_FAN];
#pragma unroll
    for (u32 q = 0; q < TK_REFILL_FAN; q++) {
        bool has = q < fan && g0 + q < play_groups;
        len0[q] = has ? tk_ld(&rcount[TK_RC(g0 + q, 0)]) : 0u;
        len1[q] = has ? tk_ld(&rcount[TK_RC(g0 + q, 1)]) : 0u;
    }
    // The workgroup's add must not overtake the count reads of its OWN later waves (every thread reads the count at the top
    // of the kernel; were this the last workgroup of its counter to add, a wave that read after the add would see the next
    // launch's band: the wrong parity, the list the running launch is writing).  The barrier puts every wave's read into the
    // memory pipe ahead of the add; step_role and play_role add behind their first barrier as well.
    if (!BULK) {
        __syncthreads();
        launch_counted<KIND>(epoch);
    }
    const u32 phase = launch_phase<KIND>(count, play_groups, kind_fan), par = phase & 1u;
    if (!BULK) {                 // empty the stretch lists
        if (tid < 2 * fan && g0 + tid / 2 < play_groups) rcount[TK_RC(g0 + tid / 2, 2 + (tid & 1))] = 0u;
    }
    u32 cum[TK_REFILL_FAN + 1];
    cum[0] = 0;
    u32 which = par ^ 1u;
    const u32 odd = 0u - par;    // (a mask, not a select between the arrays: that becomes a parity-indexed array in scratch)
#pragma unroll
    for (u32 q = 0; q < TK_REFILL_FAN; q++) cum[q + 1] = cum[q] + ((len0[q] & odd) | (len1[q] & ~odd));
    const bool any = cum[TK_REFILL_FAN] != 0;                 // (the same in every thread: nobody writes these lengths in this launch)
    // the lists of the workgroup's groups, one after the other, entry j on thread j mod nthreads; BULK: a second pass (the
    // same code: one copy of the deal) over the stretch lists in the launches that work them off
    u64 *lists = rlist;
    u32 cap = TK_REFILL_CAP;
    const bool bulk = BULK && bulk_on && phase % TK_BULK_EVERY == 0;      // (bulk_on: the env's step workgroups fill stretch lists)
#pragma nounroll
    for (u32 pass = 0; pass < (BULK ? 2u : 1u); pass++) {
        if (pass == 1) {
            if (!bulk) break;
            which = ((phase / TK_BULK_EVERY) & 1u) ^ 1u;     // the stretch before this one
            lists = elist; cap = TK_BULK_CAP;
#pragma unroll
            for (u32 q = 0; q < TK_REFILL_FAN; q++) {
                bool has = q < fan && g0 + q < play_groups;
                cum[q + 1] = cum[q] + (has ? min(tk_ld(&rcount[TK_RC(g0 + q, 2 + which)]), (u32)TK_BULK_CAP) : 0u);
            }
        }
        for (u32 j = tid; j < cum[TK_REFILL_FAN]; j += nthreads) {
            u32 q = 0;
#pragma unroll
            for (u32 r = 1; r < TK_REFILL_FAN; r++) q += j >= cum[r] ? 1u : 0u;
            u32 base = 0;
#pragma unroll
            for (u32 r = 0; r < TK_REFILL_FAN; r++) base = (r == q) ? cum[r] : base;
            u64 en = tk_ld(&lists[((int64_t)(g0 + q) * 2 + which) * cap + (j - base)]);
            deal_into_buffer(aux, (int64_t)(g0 + q) * TK_BLOCK + (u32)(en & 0xFFFF), (u32)(en >> 32), seed, offset, mix);
        }
    }
    // the lengths worked off are cleared (the one-card step's workgroups write a length only when they list something);
    // every thread has had its copies (cum[]) before the barrier
    if (any || bulk) {
        __syncthreads();
        if (any && tid < fan && g0 + tid < play_groups) rcount[TK_RC(g0 + tid, par ^ 1u)] = 0u;
        if (bulk && tid < fan && g0 + tid < play_groups) rcount[TK_RC(g0 + tid, 2 + which)] = 0u;     // (which: the stretch list's, after the second pass)
    }
}

// Play role of a Bot-policy launch (tarok_krog_random: `cards` cards per launch, the card from the in-kernel Bot
// policy, Igralec.py:158-159) for the 256 slots of play workgroup `group`: thread `tid` (0..255) plays slot
// group * 256 + tid.  (One card per launch from an external policy: step_role below.)
// HIST: also record the play history (one byte per card; tarok_create flag TAROK_HISTORY).
template <bool HIST>
__device__ __forceinline__ void play_role(
    u32 group, u32 tid,
    int64_t n, u64 seed, u64 offset, int mix, int flags, int cards, int64_t stride, TkCount count, u32 *epoch, u32 play_groups, u32 fan,
    uint8_t *__restrict__ action_out, int16_t *__restrict__ reward,
    uint8_t *__restrict__ done, uint16_t *__restrict__ trick, u64 *__restrict__ obs, uint8_t *__restrict__ hist,
    ulonglong2 *__restrict__ s01, ulonglong2 *__restrict__ s23, Aux *aux, Counters *__restrict__ cnt,
    u64 *__restrict__ gkey, u64 *rlist, u32 *rcount, u64 *__restrict__ stamps) {
    __shared__ unsigned short push_list[TK_REFILL_CAP];   // (how far ahead) * TK_BLOCK + slot in group
    __shared__ u32 push_ep[TK_BLOCK];                     // the slot's episode number at the end of the launch
    __shared__ u32 push_count;
    // Deferred scoring (the multi-card kernel): a game that ends leaves its final state in a per-wave LDS ring
    // (9 dwords) instead of being scored on the spot — with ~10 % of the slots finishing per trick the
    // scoring code (both contract families, ~250 instructions) ran for every wave on every trick with 7 of 64
    // lanes active: a third of a play wave's time at 65,536 games (profiles/r02_card_probe_before.txt).  Whenever 64 entries
    // wait they are scored in ONE pass on full lanes (drain_finished); the rest at the end of the launch.  The
    // scores go to their reward row from there and are summed per slot in LDS (sacc) for the slot's score_sum.
    __shared__ u32 finq[TK_BLOCK / 64][9][TK_FINQ];
    __shared__ int sacc[4][TK_BLOCK];
    if (tid == 0) push_count = 0;
    sacc[0][tid] = 0; sacc[1][tid] = 0; sacc[2][tid] = 0; sacc[3][tid] = 0;
    __syncthreads();
    u32 fq_head = 0, fq_n = 0;               // this wave's ring: first waiting entry, entries waiting (wave uniform)
    u32 (*fq)[TK_FINQ] = finq[tid >> 6];
    // score `cnt_` waiting entries (at most 64) of the wave's ring on dense lanes
    auto drain_finished = [&](u32 cnt_) __attribute__((always_inline)) {
        u32 lane = tid & 63;
        if (lane < cnt_) {
            u32 e = (fq_head + lane) & (TK_FINQ - 1);
            Game f;
            // (the trick-aligned loops push their C plane as they keep it, TK_C_PAD set: cleaned here, once per 64 games)
            f.A = TK_U64(fq[0][e], fq[1][e]); f.B = TK_U64(fq[2][e], fq[3][e]); f.C = TK_U64(fq[4][e], fq[5][e] & 0x3FFFFFu);
            u32 m = fq[7][e], ri = fq[8][e];
            f.talon = TK_U64(fq[6][e], (m >> 24) & 15u);
            f.contract = m & 15; f.declarer = (m >> 4) & 3; f.king = (m >> 6) & 3; f.team = (m >> 8) & 15;
            f.tl = (m >> 12) & 7; f.trick_no = (m >> 16) & 15; f.leader = (m >> 20) & 3;
            f.trick = 0; f.nt = 0; f.phase = TK_PHASE_DONE; f.error = 0; f.epar = 0; f.cprev = 0;
            u64 sc = final_scores(f);
            u32 t = ri & 0xFFFFu;
            if (reward) {
                u64 rs = sc;
                if ((flags & TAROK_REWARD_REF) && (f.contract == TK_BERAC || f.contract == TK_ODPRTI_BERAC)) {
                    int dv = f.trick_no >= 12 ? -20 : 20;                  // Igralec.py:434-437 (see the immediate path below)
                    u32 d = f.declarer;
                    rs = pack_scores(d == 0 ? (int)(int16_t)(sc & 0xFFFF) : dv, d == 1 ? (int)(int16_t)((sc >> 16) & 0xFFFF) : dv,
                                     d == 2 ? (int)(int16_t)((sc >> 32) & 0xFFFF) : dv, d == 3 ? (int)(int16_t)(sc >> 48) : dv);
                }
                reinterpret_cast<u64 *>(reward)[(int64_t)group * TK_BLOCK + t + (int64_t)(ri >> 16) * stride] = rs;
            }
            atomicAdd(&sacc[0][t], (int)(int16_t)(sc & 0xFFFF)); atomicAdd(&sacc[1][t], (int)(int16_t)((sc >> 16) & 0xFFFF));
            atomicAdd(&sacc[2][t], (int)(int16_t)((sc >> 32) & 0xFFFF)); atomicAdd(&sacc[3][t], (int)(int16_t)(sc >> 48));
        }
        fq_head = (fq_head + cnt_) & (TK_FINQ - 1);
        fq_n -= cnt_;
    };
    u64 t_real0 = 0, t_cyc0 = 0, t_play = 0;
    if (stamps) { t_real0 = __builtin_amdgcn_s_memrealtime(); t_cyc0 = __builtin_amdgcn_s_memtime(); }
    int64_t i = (int64_t)group * TK_BLOCK + tid;
    bool valid = i < n;
    int64_t ic = valid ? i : n - 1;
    Game g;
    load_game(g, s01, s23, ic);
    u64 key = gkey[ic];
    bool autoreset = (flags & TAROK_AUTO_RESET) != 0;
    // Lanes that can reach the end of their game within this launch (a game only ends on the 4th
    // card of a trick: Berac on any trick, the others in trick 12) issue their finish-path loads
    // NOW, next to the state load, instead of as a second memory round trip after the rules.
    bool berac = g.contract == TK_BERAC || g.contract == TK_ODPRTI_BERAC;
    bool spec = valid && ((g.phase == TK_PHASE_PLAY && (int)g.nt + cards >= 4 &&
                           (berac || (int)(g.trick_no * 4 + g.nt) + cards >= 48)) ||
                          g.phase == TK_PHASE_DONE);
    // Next-game lines this launch may take: the lines the previous launch put on its refill list
    // (the `cprev` farthest ahead) are being written by refill workgroups right now.
    u32 cprev0 = valid ? g.cprev : 0u;
    u32 allowed = TK_AHEAD - min(cprev0, (u32)TK_AHEAD);
    int4 acc = make_int4(0, 0, 0, 0);
    u32 cur_ep = 0;
    // (na, nb, nkey, nep1): the line of the next game (episode cur_ep + 1).  The trick-aligned loops hold this ONE
    // line: a lane that takes it fetches the next at the first card of the following trick (below), and whether a
    // lane holds its line is read off the tag (nep1 == cur_ep + 1).  The loops that are not trick-aligned have no
    // such place to fetch from and keep a second line, (na2, nb2, nkey2, nep2): the game after the next, with
    // ok1 / ok2: the line has been requested (and was one this launch may take).  A tag is compared when the line
    // is taken, so that nothing waits for the load where it is issued (line_tag).  The lines are loaded here,
    // before the loop, and inside it at a trick's first card, to be taken at its 4th.  Across the loop's back edge
    // the rule is: the TAG has landed (the 4th card votes on it on every trick), so the next trick's compare of it
    // waits for nothing.  The two pair loads issued behind the tag's are waited for only where a lane takes them;
    // after a trick in which no lane of the wave finished they are formally still in flight at the back edge and
    // are waited for inside the next fetch, whose registers they write — behind the twelve stores of a trick
    // (vmcnt counts loads and stores in order), ~1,400 cycles after they were issued: nothing stalls there.  What
    // must not happen is a load ISSUED late in a trick and consumed early in the next: every iteration would
    // wait for the previous iteration's stores
    ulonglong2 na = make_ulonglong2(0, 0), nb = na, na2 = na, nb2 = na;
    u64 nkey = 0, nkey2 = 0;
    u32 nep1 = 0, nep2 = 0;
    bool ok1 = false, ok2 = false;
    auto line_tag = [&](bool &ok, u32 &nep, u32 tag) __attribute__((always_inline)) { nep = tag; ok = true; };
    // a line in three loads: the two packed pairs, and the key with the tag behind it — twelve bytes of the line's
    // third 16, in three registers (a 16-byte load's fourth register is dead from the start: the allocator hands it
    // to the next instruction that needs one, which then waits for the load to land — at the card that issued it)
    static_assert(offsetof(AuxLine, nkey) == 32 && offsetof(AuxLine, nep) == 40, "key and tag share the line's third 16 bytes");
    auto load_line = [&](const AuxLine *ln, ulonglong2 &a, ulonglong2 &b, u64 &k, bool &ok, u32 &nep) __attribute__((always_inline)) {
        a = ln->n01; b = ln->n23;
        uint3 kt = *reinterpret_cast<const uint3 *>(__builtin_assume_aligned(&ln->nkey, 16));
        k = TK_U64(kt.x, kt.y);
        line_tag(ok, nep, kt.z);
    };
    // With auto-reset a lane that is in play stays in play (a finished game is replaced within the same card), and
    // games are whole tricks long: a wave whose lanes all start a launch of whole tricks at a trick boundary plays
    // the trick-aligned loop (below) — known here, where it decides how many lines are loaded ahead.
    const bool all_play = autoreset && __ballot(valid && g.phase == TK_PHASE_PLAY) == ~0ULL;
    // (the trick-aligned loops address the action and done rows by a 32-bit element offset, see out_b below: a launch whose
    // last row would not fit one plays the loop that is not trick-aligned — more than twenty million games at 192 cards)
    const bool aligned = all_play && (cards & 3) == 0 && __ballot(g.nt != 0) == 0 &&
                         (u64)stride <= 0xFFFFFFFFull && (u64)stride * (u32)cards + (u64)n <= 0xFFFFFFFFull;
    if (spec) {
        acc = cnt[i].score_sum;
        cur_ep = cnt[i].episode;
        if (autoreset && allowed > 0) {
            load_line(&aux[i].line[TK_LINE(g.epar + 1)], na, nb, nkey, ok1, nep1);
            if (!aligned && allowed > 1 && cards > 4)          // a Berac can be over after 4 cards
                load_line(&aux[i].line[TK_LINE(g.epar + 2)], na2, nb2, nkey2, ok2, nep2);
        }
    }
    TK_WAIT_LOADS();                        // nothing in flight when the loop starts (see above)
    u32 par = launch_phase<1>(count, play_groups, fan) & 1u;     // (`count` was requested before the state: it has arrived with it)
    launch_counted<1>(epoch);
    g.cprev = 0;
    u32 consumed = 0;                       // games swapped in / dealt during this launch
    bool resync = false;                    // a line that should have been usable was not: refill them all
    bool blocked = false;                   // a game was dealt in place: no more swap-ins in this launch
    bool acc_dirty = false, seats_dirty = false, touched = false;
    // the legal mask written into the observation after card c is the one the policy needs for
    // card c+1: computed once per card, carried in a register
    u64 legal = (valid && g.phase == TK_PHASE_PLAY) ? legal_now(g) : 0;
    u64 c_lead = 0;
    u32 legal_hi = 0;                        // trick-aligned loops, cards 1..3: which word of `legal` holds the cards (legal_mask_follow)
    // trick-aligned loops, carried from card to card: the RNG counter of the card to play (rng_ctr(128 + cards played)) and
    // the seat / position half of the observation word (obs_carry) — each moves by a constant per card
    u32 rctr = 0, ocar = 0;
    // trick-aligned loops, carried too: what the rules ask of the contract (FamilyWord: set where a game is taken, as rctr is) and
    // of the card led (LeadWord: set at a trick's first card; with it g.trick is not read in these loops).  The game's error
    // bit rides in ocar, already shifted (obs_carry), and the smears of the seat to play are read off ocar's top bits
    FamilyWord fam = FamilyWord{0u};
    LeadWord led = LeadWord{0u};
    u32 resync_v = 0;                       // `resync` of the fast-renewal loop, as a number (a bool carried through a loop is a
                                             // lane mask, merged with three scalar instructions at every join, used or not)
    // the fast-renewal loop's `allowed` and `blocked` in one number: how many games of this launch the lane may take
    // from lines — none for a lane that cannot finish in this launch (its counters are not loaded), none any more
    // once a game was dealt in place
    u32 lim = spec ? allowed : 0u;
    // trick-aligned loops: where the card's output rows go.  The action and done rows share ONE 32-bit element offset per
    // lane (scalar base + 32-bit lane offset: the store forms its address itself), one add per card for both; the
    // observation row keeps a 64-bit pointer (eight times the offset passes 2^32 at four million games), one add per card.
    // Eight address instructions per trick for its twelve stores, not fourteen
    u32 out_b = (u32)i;
    u64 *out_obs = obs + i;
    // fill the line buffers of the lanes that lack them (lacks: the next game's, lacks2: the one after it)
    auto fetch_lines = [&](bool lacks, bool lacks2) __attribute__((always_inline)) {
        if (lacks) load_line(&aux[i].line[TK_LINE(cur_ep + 1)], na, nb, nkey, ok1, nep1);
        if (lacks2) load_line(&aux[i].line[TK_LINE(cur_ep + 2)], na2, nb2, nkey2, ok2, nep2);
    };
    auto play_card = [&](auto all_tag, auto nt_tag, auto std_tag, int64_t row, int ci) __attribute__((always_inline)) {
        // ALL: every lane of the wave is a valid slot with a game in play (wave uniform, see below):
        // no per-lane predicates around the rules and the output stores.
        // NT >= 0: moreover every lane is at card NT of its trick: the constant propagates through
        // the rules (no trick-end test on cards 0..2, constant shifts, "somebody led" known)
        // STD: the usual set of outputs of a rollout — action_out and done given, trick not — known for the
        // whole launch: no pointer tests per card (two scalar instructions each: as dear as vector ones here)
        constexpr bool ALL = decltype(all_tag)::value;
        constexpr int NT = decltype(nt_tag)::value;
        constexpr bool STD = decltype(std_tag)::value;
        if constexpr (NT >= 0) g.nt = (u32)NT;
        // Trick-aligned loops: a lane that took its line at a 4th card fetches the line of its next game HERE, at the
        // first card of the following trick — three cards (~1,400 cycles) before a game can end and take it, even a
        // Berac that is over after one trick: the memory round trip hides behind the rules, and the compiler's
        // wait at the first use counts past the stores issued since.  One line is therefore enough: a second,
        // buffered one would be fetched at the same card and waited for at the same place.  (A lane's `consumed`
        // only moves at a 4th card, so a lane that still lacks a line at the 4th card could not have fetched one:
        // no fetch on the spot in these loops.)  With four waves on a SIMD the other waves hide the round trip of
        // a fetch on the spot, and the earlier, more frequent fetches only cost instructions (4 M games: -11 %).
        constexpr bool TOP_UP_EARLY = ALL && NT == 0;
        constexpr bool TOP_UP_LATE = !(ALL && NT == 3);
        if constexpr (TOP_UP_EARLY) {
            // (Which lane holds its line is read off the tag: nep1 is the number of the lane's next game, or the lane
            // has no line.  No wave-uniform "somebody swapped" flag in front: with ~10 % of the slots finishing per
            // trick it is set on nearly every trick.  The line's index follows the game's epar = TK_LINE(cur_ep): a
            // compare, not a division by fourteen.  No `consumed >= 1` in the condition: it would only keep a lane whose
            // PRELOADED line carries a stale tag — after one-card launches or a change of the refill fan, a handful of
            // launches in an env's life — from asking for that line again, three loads per trick under its own exec
            // bit until it finishes, deals in place and drops to lim = 0.  The tag stays stale (this launch's refill
            // workgroups write only lines that `lim` excludes), so results are the same; the compare and its mask
            // would be paid by every wave on every trick of every launch.)
            if (nep1 != cur_ep + 1 && consumed < lim) {
                u32 off = g.epar + 1 >= (u32)TK_AHEAD ? 0u : (g.epar + 1) * (u32)sizeof(AuxLine);
                load_line(reinterpret_cast<const AuxLine *>(reinterpret_cast<const char *>(aux[i].line) + off), na, nb, nkey, ok1, nep1);
            }
        }
        const bool v = ALL ? true : valid;
        const bool play = ALL ? true : (valid && g.phase == TK_PHASE_PLAY);
        // (trick-aligned loops: g.C carries TK_C_PAD from the first card to the last, see tricks() below)
        constexpr bool ALIGNED = ALL && NT >= 0;
        u32 a;
        // (trick-aligned loops: the card's RNG counter is carried, one add per card, not rebuilt from trick_no and nt)
        if constexpr (ALL && NT >= 1) a = policy_action_follow(key, RngCtr{rctr}, TK_LO(legal) | TK_HI(legal), legal_hi);
        else if constexpr (ALIGNED) a = policy_action(key, RngCtr{rctr}, legal);
        else a = play ? policy_action(key, g.trick_no * 4 + g.nt, legal) : 255u;
        if constexpr (ALIGNED) rctr += TK_RNG_STEP;       // (the 4th card's renewal region resets it for a fresh game)
        u64 scores = 0;
        u32 trick_info = 0;
        int res = -2;
        const u32 pos = g.trick_no * 4 + g.nt;            // cards played so far in this game
        // (trick-aligned loops: the C plane as the trick's first card finds it — what it gains until the 4th card is the trick)
        if constexpr (ALL && NT == 0) c_lead = g.C;
        const u64 *lead_plane = (ALL && NT >= 0) ? &c_lead : nullptr;
        if constexpr (ALL && NT == 0) led = lead_word(a);
        if constexpr (ALIGNED) res = apply_step<true, true, true>(g, a, scores, trick_info, !STD && trick != nullptr, lead_plane, fam, led);
        else if (play) res = apply_step<true, true>(g, a, scores, trick_info, !STD && trick != nullptr, lead_plane);
        bool fin = res == 1;
        // the play history (zgodovina, Klop.py:63 / Navadna_igra.py:127): card `pos` of the game, one byte,
        // write-only here; only the reference-layout observation (k_observe_ref) reads it
        if (HIST && hist && play && res >= 0) hist[(int64_t)pos * n + i] = (uint8_t)a;
        // (trick-aligned loops: every lane plays whole tricks — both are set once, before the loop; a per-lane
        // flag carried through a loop is a lane mask that costs three scalar instructions per update)
        if constexpr (!(ALL && NT >= 0)) {
            touched = touched || res != -2;
            seats_dirty = seats_dirty || (res >= 0 && g.nt == 0);
        }
        if constexpr (ALIGNED) {
            if (STD || action_out) TK_STREAM_STORE(&action_out[out_b], (uint8_t)a);
            if (!STD && trick) TK_STREAM_STORE(&trick[out_b], (uint16_t)trick_info);
        } else if (v) {
            if (STD || action_out) TK_STREAM_STORE(&action_out[row], (uint8_t)a);
            if (!STD && trick) TK_STREAM_STORE(&trick[row], (uint16_t)trick_info);
        }
        // (cards 0..2 of a trick cannot end a game: no finish / renewal code in their copies)
        constexpr bool CAN_END = !(ALL && NT >= 0 && NT < 3);
        // the trick-aligned loop: queue + renewal of the finishing lanes in one exec region, every per-lane fact
        // kept in vector registers (below)
        constexpr bool FAST_RENEW = ALL && NT == 3;
        auto push_finished = [&](u64 fm, u32 slot0) __attribute__((always_inline)) {   // (lanes with fin; slot0: first free ring entry)
            u32 e = (slot0 + __builtin_amdgcn_mbcnt_hi((u32)(fm >> 32), __builtin_amdgcn_mbcnt_lo((u32)fm, 0))) & (TK_FINQ - 1);
            fq[0][e] = TK_LO(g.A); fq[1][e] = TK_HI(g.A); fq[2][e] = TK_LO(g.B); fq[3][e] = TK_HI(g.B);
            fq[4][e] = TK_LO(g.C); fq[5][e] = TK_HI(g.C); fq[6][e] = TK_LO(g.talon);
            // (one v_lshl_or per field: left alone the compiler builds a tree of shifts and v_or3, twelve instructions)
            u32 m = (g.declarer << 4) | g.contract;      TK_KEEP_VGPR(m);
            m = (g.king << 6) | m;                       TK_KEEP_VGPR(m);
            m = (g.team << 8) | m;                       TK_KEEP_VGPR(m);
            m = (g.tl << 12) | m;                        TK_KEEP_VGPR(m);
            m = (g.trick_no << 16) | m;                  TK_KEEP_VGPR(m);
            m = (g.leader << 20) | m;                    TK_KEEP_VGPR(m);
            fq[7][e] = (TK_HI(g.talon) << 24) | m;
            fq[8][e] = ((u32)ci << 16) | tid;
        };
        auto swap_in = [&]() __attribute__((always_inline)) {                   // (lanes that hold their next game's line)
            unpack_fresh(g, na.x, na.y, nb.x, nb.y);  // carries epar of the new game
            if constexpr (ALIGNED) g.C |= TK_C_PAD;
            key = nkey;
            // (trick-aligned loops: nothing moves up — the tag left behind is the game just taken, so the lane
            // reads as being without a line until the next trick's first card has fetched one)
            if constexpr (!ALIGNED) {
                na = na2; nb = nb2; nkey = nkey2;
                nep1 = nep2;
            }
        };
        // a game dealt here and now, for the lanes with deal_here (all 64 lanes must come along: deal_wave)
        auto deal_in_place = [&](bool deal_here, Game &gd, u64 &kd) __attribute__((always_inline)) {
            u64 pend = __ballot(deal_here);
            if (TK_RARE(pend != 0)) {
                u64 dkey = 0;
                if (deal_here) dkey = game_key(seed, offset + (u64)i, cur_ep + 1);
                u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, tal = 0;
                u32 lane = __lane_id();
                while (pend) {
                    int l = __builtin_ctzll(pend);
                    pend &= pend - 1;
                    u32 klo = (u32)__builtin_amdgcn_readlane((int)(u32)dkey, l);
                    u32 khi = (u32)__builtin_amdgcn_readlane((int)(u32)(dkey >> 32), l);
                    u64 w0, w1, w2, w3, wt;
                    deal_wave(klo, khi, w0, w1, w2, w3, wt);
                    if (lane == (u32)l) { h0 = w0; h1 = w1; h2 = w2; h3 = w3; tal = wt; }
                }
                if (deal_here) {
                    u32 cc, d, k;
                    sample_setup(dkey, mix, cc, d, k);
                    setup_game(gd, h0, h1, h2, h3, tal, cc, d, k);
                    gd.epar = TK_LINE(cur_ep + 1); gd.cprev = 0;
                    if (gd.phase == TK_PHASE_EXCHANGE) bot_exchange(gd, dkey);
                    kd = dkey;
                }
            }
        };
        if constexpr (FAST_RENEW) {
            // Every lane is in play, so the lanes to renew are the finishing ones, and a lane can take its next game
            // from the line it holds exactly when that line's tag is the game's number (a tag never matches a later
            // game, and a line with the right tag IS the game: no "requested" / "dealt in place" flags here).  A
            // finishing lane without its line is rare: its game is dealt on the spot INTO the line registers, so that
            // there is one renewal path: queue entry, swap and counters of the finishing lanes in one exec region, all
            // on vector registers.  (Per-lane flags kept as lane masks cost three scalar instructions per update
            // inside a divergent region, and every compare -> mask -> select hop stalls a lone wave: tools/valu_issue.)
            u64 fm = __ballot(fin);
            // (voted on every trick, not only where a game ends: the tag of a line fetched at the first card has then
            // landed before the loop's back edge whether or not a lane finishes, and the next trick's compare of it
            // waits for nothing.  The line's pairs are waited for where a lane takes them; after a trick without a
            // finish they cross the back edge and are waited for at the next fetch — behind the twelve stores of a
            // trick, which have long gone: the relaxed back-edge rule stated at the line registers above.)
            const u64 nol = __ballot(nep1 != cur_ep + 1);
            if (TK_USUAL(fm != 0)) {                                      // (wave uniform)
                if (TK_RARE(fq_n >= 64)) drain_finished(64);              // room for 64 more: fewer than 64 wait now
                const u32 slot0 = fq_head + fq_n;                         // (scalar bookkeeping outside the exec region)
                fq_n += (u32)__popcll(fm);
                // (a vote on ONE compare, and-ed with the finishing lanes as a scalar: see apply_step's last lines)
                if (TK_RARE((fm & nol) != 0)) {
                    bool lineless = fin && nep1 != cur_ep + 1;
                    // ran out of usable lines (the next ones are being re-dealt right now: the usual
                    // bookkeeping stays valid) vs a line that should have been there and is not
                    resync_v |= (lineless && consumed < lim) ? 1u : 0u;
                    lim = lineless ? 0u : lim;                            // (no more fetches for this lane in this launch)
                    Game d = g;
                    u64 dk = key;
                    deal_in_place(lineless, d, dk);
                    if (lineless) { pack(d, na.x, na.y, nb.x, nb.y); nkey = dk; nep1 = cur_ep + 1; }
                }
                if (fin) { push_finished(fm, slot0); swap_in(); cur_ep++; consumed++; rctr = rng_ctr(128u).v; fam = family_word(g.contract); }
            }
        }
        if constexpr (CAN_END && !FAST_RENEW) {
            u64 fm = __ballot(fin);
            if (TK_USUAL(fm != 0)) {                                      // (wave uniform)
                if (TK_RARE(fq_n >= 64)) drain_finished(64);                       // room for 64 more: fewer than 64 wait now
                if (fin) push_finished(fm, fq_head + fq_n);
                fq_n += (u32)__popcll(fm);
            }
        }
        if (CAN_END && !FAST_RENEW && (ALL || autoreset)) {  // (ALL implies auto-reset, and every lane was in play: done = just finished)
            bool renew = ALL ? fin : (v && g.phase == TK_PHASE_DONE);
            if (TK_USUAL(__ballot(renew) != 0)) {
                // Loops that are not trick-aligned: a third or later game of a launch (the two preloaded lines
                // are used up) is fetched on the spot: a memory round trip (~550 cycles) that nothing hides.  So
                // when one lane has to, EVERY lane that has used its lines up takes its next games' lines along —
                // finishing or not: the one wait serves them all.
                if constexpr (TOP_UP_LATE) {
                    bool lacks = spec && !blocked && !ok1 && consumed >= 1 && consumed < allowed;
                    if (TK_RARE(__ballot(renew && lacks) != 0)) {
                        bool lacks2 = spec && !blocked && !ok2 && consumed >= 1 && consumed + 1 < allowed;
                        fetch_lines(lacks, lacks2);
                        TK_WAIT_LOADS();
                    }
                }
                bool swap = renew && !blocked && ok1 && nep1 == cur_ep + 1;
                if (swap) {
                    swap_in();
                    ok1 = ok2 && consumed + 1 < allowed;
                    ok2 = false;
                }
                bool deal_here = renew && !swap;             // line missing, stale or being re-dealt
                // ran out of usable lines (the next ones are being re-dealt right now: the usual
                // bookkeeping stays valid) vs a line that should have been there and is not
                if (deal_here && consumed < allowed) resync = true;
                if (deal_here) blocked = true;
                deal_in_place(deal_here, g, key);
                if (renew) { cur_ep++; consumed++; seats_dirty = true; }
            }
        }
        // (ALL: a finished game has been replaced just above, so every lane is in play again)
        // (trick-aligned loops: the seat and position bits are carried, one add per card; after the 4th card the seat to play
        // is the trick's winner, or a fresh game's leader, and the error bit may be a fresh game's: rebuilt there.  The hand
        // to play next is the hand of the seat in the word's top bits)
        if constexpr (ALIGNED && NT < 3) ocar += TK_OBS_CARD;
        else if constexpr (ALIGNED) ocar = obs_carry(g.leader, g.trick_no << 2, g.error);
        if constexpr (ALIGNED && NT < 3) legal = legal_mask_follow(hand_of<true>(g, obs_carry_ma(ocar), obs_carry_mb(ocar)), led, fam, legal_hi);
        else if constexpr (ALIGNED) legal = legal_mask(hand_of<true>(g, obs_carry_ma(ocar), obs_carry_mb(ocar)), fam);
        else legal = (ALL || (v && g.phase == TK_PHASE_PLAY)) ? legal_now(g) : 0;
        // (ALL: res is 0 or 1 — the number itself goes into the observation's bit 62 and the done row, no selects)
        const u32 fin01 = ALL ? (u32)res : (fin ? 1u : 0u);
        if constexpr (ALIGNED) {
            TK_STREAM_STORE(out_obs, obs_word_with(ocar, fin01, legal));
            if (STD || done) TK_STREAM_STORE(&done[out_b], (uint8_t)fin01);
            out_b += (u32)stride; out_obs += stride;          // (the card's last stores: on to the next card's row)
        } else if (v) {
            TK_STREAM_STORE(&obs[row], obs_word_with<true>(g, false, legal) | ((u64)(ALL ? fin01 : ((fin || g.phase == TK_PHASE_DONE) ? 1u : 0u)) << 62));
            if (STD || done) TK_STREAM_STORE(&done[row], (uint8_t)fin01);
        }
    };
    // "Every lane of the wave valid and in play" (all_play, above) holds for the whole launch: one of two
    // separate loops (a choice per card made the loop body slower than either).  Lanes that start a launch of
    // whole tricks at a trick boundary stay trick-aligned too (aligned): third loop, four specialised cards per trick.
    int64_t row = i;
    typedef std::integral_constant<int, -1> nt_any;
    if (all_play) {
        if (aligned) {
            auto tricks = [&](auto std_tag) __attribute__((always_inline)) {
                touched = true; seats_dirty = true;          // (cards >= 4: every lane plays a whole trick)
                // the C plane's high word keeps the ten bits above the deck set for the length of the loop: every hand
                // comes out of ~C without them (hand_of<true>).  The trick's cards are the plane's gain (c_lead carries
                // the bits too); the plane is cleaned where it leaves: below, and where a finished game is scored.
                g.C |= TK_C_PAD;
                rctr = rng_ctr(128u + g.trick_no * 4).v;
                ocar = obs_carry(g.leader, g.trick_no << 2, g.error);
                fam = family_word(g.contract);
                // (these copies address their rows by out_b / out_obs, advanced inside the card: `row` is not read)
                for (int c = 0; c < cards; c += 4) {
                    play_card(std::true_type{}, std::integral_constant<int, 0>{}, std_tag, row, c);
                    play_card(std::true_type{}, std::integral_constant<int, 1>{}, std_tag, row, c + 1);
                    play_card(std::true_type{}, std::integral_constant<int, 2>{}, std_tag, row, c + 2);
                    play_card(std::true_type{}, std::integral_constant<int, 3>{}, std_tag, row, c + 3);
                }
                g.C &= TK_DECK;
            };
            if (action_out && done && !trick) tricks(std::true_type{});
            else tricks(std::false_type{});
        } else {
            for (int c = 0; c < cards; c++, row += stride) play_card(std::true_type{}, nt_any{}, std::false_type{}, row, c);
        }
    } else {
        for (int c = 0; c < cards; c++, row += stride) play_card(std::false_type{}, nt_any{}, std::false_type{}, row, c);
    }
    // ---- schedule the refills: after consuming, the slot must again hold episodes cur+1 .. cur+TK_AHEAD.
    // Each swap-in vacated one line (the others stay valid): the last np episodes are new;
    // a game dealt in place: all of them.
    while (fq_n) drain_finished(min(fq_n, 64u));                          // (at most two passes: fewer than 128 wait)
    __builtin_amdgcn_s_waitcnt(0xC07F);                                   // the wave's LDS adds have landed (lgkmcnt(0))
    {
        int4 sa = make_int4(sacc[0][tid], sacc[1][tid], sacc[2][tid], sacc[3][tid]);
        if (sa.x | sa.y | sa.z | sa.w) { acc.x += sa.x; acc.y += sa.y; acc.z += sa.z; acc.w += sa.w; acc_dirty = true; }
    }
    u32 np = (resync || resync_v != 0) ? (u32)TK_AHEAD : min(consumed, (u32)TK_AHEAD);
    if (valid) {
        g.cprev = np;                        // the next launch must not read those lines
        if (acc_dirty) cnt[i].score_sum = acc;
        if (consumed) { cnt[i].episode = cur_ep; gkey[i] = key; }
        if (touched || consumed || cprev0 != np) store_game(g, s01, s23, i, seats_dirty || cprev0 != np);
    }
    if (stamps) t_play = __builtin_amdgcn_s_memtime() - t_cyc0;
    if (valid && np) {
        u32 pos = atomicAdd(&push_count, np);
        push_ep[tid] = cur_ep;
        for (u32 j = 0; j < np; j++) push_list[pos + j] = (unsigned short)(j * TK_BLOCK + tid);
    }
    __syncthreads();
    u32 total = push_count;
    u64 *lst = rlist + ((int64_t)group * 2 + par) * TK_REFILL_CAP;
    for (u32 j = tid; j < total; j += TK_BLOCK) {                  // list entry: episode to deal << 32 | slot in group
        u32 en = push_list[j], t = en % TK_BLOCK;
        lst[j] = ((u64)(push_ep[t] + TK_AHEAD - en / TK_BLOCK) << 32) | t;
    }
    if (tid == 0) rcount[TK_RC(group, par)] = total;
    if (stamps && (tid & 63) == 0) {     // diagnostics only
        u64 w = (u64)i >> 6;
        stamps[3 * w + 0] = t_real0;
        stamps[3 * w + 1] = __builtin_amdgcn_s_memrealtime();
        stamps[3 * w + 2] = ((__builtin_amdgcn_s_memtime() - t_cyc0) << 32) | (t_play & 0xFFFFFFFFULL);
    }
}

// The Bot-policy kernel (tarok_krog_random; every batch size): ~165 VGPRs, nothing spills inside the card loops —
// still three waves per SIMD, and where the batch puts one wave on a SIMD (65,536 games) a scratch reload would
// be a memory round trip that nothing hides; the next games' lines are topped up early and the usual path falls
// through its branches.  (Rounds 1-2 also shipped a 128-VGPR build of it, four waves per SIMD, slower at every
// batch size — same-box medians, G steps/s, wide | narrow: 262,144 games 160.9 | 155.3, 1 M 163.9 | 146.0,
// 4 M 175.9 | 169.3 — and selectable only through an environment variable: removed in round 3.)
// HIST: also record the play history (one byte per card; tarok_create flag TAROK_HISTORY).
#define TK_PLAY_ARGS                                                                                                             \
    int64_t n, u64 seed, u64 offset, int mix, int flags, int cards, int64_t stride, u32 play_groups, u32 *epoch, u32 fan,         \
        uint8_t *__restrict__ action_out, int16_t *__restrict__ reward,                                                           \
        uint8_t *__restrict__ done, uint16_t *__restrict__ trick, u64 *__restrict__ obs, uint8_t *__restrict__ hist,              \
        ulonglong2 *__restrict__ s01, ulonglong2 *__restrict__ s23, Aux *aux, Counters *__restrict__ cnt,                         \
        u64 *__restrict__ gkey, u64 *rlist, u32 *rcount, u64 *__restrict__ stamps
template <bool HIST>
TK_KERNEL(TK_BLOCK, 168) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_play_wide(TK_PLAY_ARGS) {
    TK_VGPR_TOP(168, 167);
    TkCount count = launch_count<1>(epoch, play_groups);
    if (blockIdx.x >= play_groups)
        refill_role<false>(blockIdx.x - play_groups, threadIdx.x, TK_BLOCK, seed, offset, mix, play_groups, count, epoch, fan, false, aux, rlist, rcount, nullptr);
    else {
        play_role<HIST>(blockIdx.x, threadIdx.x, n, seed, offset, mix, flags, cards, stride, count, epoch, play_groups, fan,
                        action_out, reward, done, trick, obs, hist, s01, s23, aux, cnt, gkey, rlist, rcount, stamps);
    }
}

// A game dealt here and now by the wave (deal_wave: all 64 lanes must come along) for the lanes with deal_here:
// episode `ep` of slot i.  The rare path of a renewal: the slot's next-game line is missing or being re-dealt.
__device__ __forceinline__ void deal_in_place_wave(bool deal_here, Game &gd, u64 &kd, u64 seed, u64 offset, int64_t i, u32 ep, int mix) {
    u64 pend = __ballot(deal_here);
    if (pend == 0) return;
    u64 dkey = 0;
    if (deal_here) dkey = game_key(seed, offset + (u64)i, ep);
    u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, tal = 0;
    u32 lane = __lane_id();
    while (pend) {
        int l = __builtin_ctzll(pend);
        pend &= pend - 1;
        u32 klo = (u32)__builtin_amdgcn_readlane((int)(u32)dkey, l);
        u32 khi = (u32)__builtin_amdgcn_readlane((int)(u32)(dkey >> 32), l);
        u64 w0, w1, w2, w3, wt;
        deal_wave(klo, khi, w0, w1, w2, w3, wt);
        if (lane == (u32)l) { h0 = w0; h1 = w1; h2 = w2; h3 = w3; tal = wt; }
    }
    if (deal_here) {
        u32 cc, d, k;
        sample_setup(dkey, mix, cc, d, k);
        setup_game(gd, h0, h1, h2, h3, tal, cc, d, k);
        gd.epar = TK_LINE(ep); gd.cprev = 0;
        if (gd.phase == TK_PHASE_EXCHANGE) bot_exchange(gd, dkey);
        kd = dkey;
    }
}

// THE ONE-CARD STEP (tarok_step, tarok_step_random, the env half of tarok_policy_step): the surface an external
// policy drives, one card of every game per launch, the state through HBM on every card — the path SURVEY 8d's
// 54 B/step describe.  Same results and the same refill protocol as play_role with cards = 1 (launches of both
// kinds mix freely), but compiled on its own: no card loops, no scoring queue, no scratch — the generic kernel's
// 128-VGPR build spilled twelve dwords per lane on this path, and a spilled dword is a store to memory: 47 of
// the 82 bytes per step it wrote (profiles/r03_step_ledger.txt).
//   Reads:  play pair 16 + seat pair 16 + the card 1 (RANDOM: the game's RNG key 8 instead).
//   Writes: play pair 16 + observation word 8 (+ done 1, action 1, trick 2 where asked for);
//           the seat pair (16) only by the lanes whose trick this card completed: every 4th card.
//   A game that ENDS also touches its slot's Counters (32 B read, 32 B written), takes its successor from the
//   slot's next-game line (64 B read), writes the successor's RNG key and puts one entry on the refill list.
// Finished games are scored on DENSE lanes: about a tenth of the slots end a game on a trick's 4th card, so every
// wave would run the scoring code (both contract families, ~270 instructions) for six active lanes — measured at
// 4 M games, the finishing lanes of a mixed batch cost 116 ps each against 40 ps in an all-Klop batch, where all
// lanes end together (profiles/r03_step_durations.txt).  A lane whose game ends leaves the final state and the
// slot's score sums in a workgroup-wide LDS list (FINQ_WORDS words per entry) and goes on to the renewal; after
// the role's one barrier the first threads of the workgroup score the list, one entry per lane, and write the
// reward rows and the score sums.  Nothing a lane does after the card depends on the scores.
// Only the lanes whose game DID end load those, after the rules (the scoring list is filled meanwhile).  Rounds 1-2
// had every lane that CAN end its game with this card — 4th card of a Berac trick or of a twelfth trick, a fifth of
// the lanes of such a launch — issue them speculatively next to the state load: 5.3 B/step more read traffic at
// 4 M games, and no faster at any batch size, 65,536 games included (profiles/r03_ab_step.txt).
#define FINQ_WORDS 13
template <bool RANDOM, bool LAZY>
__device__ __forceinline__ void step_role(
    u32 group, u32 tid, bool active, u32 a_reg, bool lazy_on,
    int64_t n, u64 seed, u64 offset, int mix, int flags, TkCount count, u32 *epoch, u32 play_groups, u32 fan,
    const uint8_t *__restrict__ action_in, uint8_t *__restrict__ action_out, int16_t *__restrict__ reward,
    uint8_t *__restrict__ done, uint16_t *__restrict__ trick, u64 *__restrict__ obs, uint8_t *__restrict__ hist,
    ulonglong2 *__restrict__ s01, ulonglong2 *__restrict__ s23, Aux *aux, Counters *__restrict__ cnt,
    u64 *__restrict__ gkey, u64 *rlist, u32 *rcount, u64 *elist,
    u32 (*__restrict__ finq)[TK_BLOCK] /* LDS [FINQ_WORDS][TK_BLOCK] */) {
    __shared__ unsigned short push_list[TK_REFILL_CAP];   // (how far ahead) * TK_BLOCK + slot in group
    __shared__ u32 push_ep[TK_BLOCK];                     // the slot's episode number at the end of the launch
    __shared__ u32 push_count, fin_count, late_count;
    __shared__ u64 late_list[LAZY ? TK_BLOCK : 1];        // LAZY: entries for the stretch list (refill_role), one per slot at most
    const bool lazy = LAZY && lazy_on;                    // (LAZY: the kernel has the stretch lists at all; lazy_on: this env uses them)
    if (tid == 0) { push_count = 0; fin_count = 0; late_count = 0; }
    // (lazy) how full the two stretch lists of this group are: asked for now by every thread (one address per workgroup),
    // looked at when the launch's entries go out — no broadcast, no barrier of its own
    u32 efill0 = 0, efill1 = 0;
    if (lazy) { efill0 = tk_ld(&rcount[TK_RC(group, 2)]); efill1 = tk_ld(&rcount[TK_RC(group, 3)]); }
    __syncthreads();
    int64_t i = (int64_t)group * TK_BLOCK + tid;
    bool valid = active && i < n;
    int64_t ic = valid ? i : n - 1;
    Game g;
    load_game(g, s01, s23, ic);
    u64 key = 0;
    u32 a = 255;
    if (RANDOM) key = gkey[ic]; else a = action_in ? action_in[ic] : a_reg;
    const bool autoreset = (flags & TAROK_AUTO_RESET) != 0;
    // next-game lines this launch may take: the `cprev` farthest ahead are being re-dealt right now (play_role)
    const u32 cprev0 = valid ? g.cprev : 0u;
    const u32 allowed = TK_AHEAD - min(cprev0, (u32)TK_AHEAD);
    int4 acc = make_int4(0, 0, 0, 0);
    u32 cur_ep = 0;
    ulonglong2 na = make_ulonglong2(0, 0), nb = na;
    u64 nkey = 0;
    u32 ntag = 0;
    bool have_line = false;
    auto load_finish = [&](bool need) __attribute__((always_inline)) {
        if (need) {
            acc = cnt[i].score_sum;
            cur_ep = cnt[i].episode;
            if (autoreset && allowed > 0) {
                const AuxLine *ln = &aux[i].line[TK_LINE(g.epar + 1)];
                na = ln->n01; nb = ln->n23; nkey = ln->nkey; ntag = ln->nep;
                have_line = true;
            }
        }
    };
    launch_counted<LAZY ? 0 : 1>(epoch);     // (issued BEFORE the count is waited for: its round trip runs beside the state's)
    g.cprev = 0;
    // ---- the card: krog's body (Klop.py:47-79, Navadna_igra.py:115-141), apply_step
    const bool play = valid && g.phase == TK_PHASE_PLAY;
    const u32 pos = g.trick_no * 4 + g.nt;                // cards played so far in this game
    if (RANDOM) a = play ? policy_action(key, pos, legal_now(g)) : 255u;
    u64 scores = 0;
    u32 trick_info = 0;
    int res = -2;
    // (a finished game is scored after the barrier, from its final state, on dense lanes)
    if (play) res = apply_step<RANDOM, true>(g, a, scores, trick_info, trick != nullptr, nullptr);
    const bool fin = res == 1;
    // the play history (zgodovina, Klop.py:63 / Navadna_igra.py:127): write-only here
    if (hist && play && res >= 0) hist[(int64_t)pos * n + i] = (uint8_t)a;
    bool seats_dirty = res >= 0 && g.nt == 0;
    if (valid) {
        if (RANDOM && action_out) TK_STREAM_STORE(&action_out[i], (uint8_t)a);
        if (trick) TK_STREAM_STORE(&trick[i], (uint16_t)trick_info);
    }
    const bool renew = autoreset && valid && g.phase == TK_PHASE_DONE;     // (also a game finished by an earlier launch)
    load_finish(fin || renew);
    if (fin) {                                            // the final state goes on the scoring list (the loads above are in flight)
        u32 e = atomicAdd(&fin_count, 1u);
        finq[0][e] = TK_LO(g.A); finq[1][e] = TK_HI(g.A); finq[2][e] = TK_LO(g.B); finq[3][e] = TK_HI(g.B);
        finq[4][e] = TK_LO(g.C); finq[5][e] = TK_HI(g.C); finq[6][e] = TK_LO(g.talon);
        finq[7][e] = g.contract | (g.declarer << 4) | (g.king << 6) | (g.team << 8) | (g.tl << 12) | (g.trick_no << 16) | (g.leader << 20) |
                     (TK_HI(g.talon) << 24);
        finq[8][e] = tid;
        finq[9][e] = (u32)acc.x; finq[10][e] = (u32)acc.y; finq[11][e] = (u32)acc.z; finq[12][e] = (u32)acc.w;
    }
    // ---- auto-reset: the successor comes out of the slot's next-game line (valid iff its tag is the game's
    // number); without a usable line the wave deals the game here and the slot's lines are all refilled
    u32 consumed = 0;
    bool resync = false;
    if (__ballot(renew) != 0) {                           // (wave uniform: deal_in_place_wave needs every lane)
        bool swap = renew && have_line && ntag == cur_ep + 1;
        if (swap) { unpack_fresh(g, na.x, na.y, nb.x, nb.y); key = nkey; }
        bool deal_here = renew && !swap;
        resync = deal_here && allowed > 0;                // a line that should have been usable was not
        deal_in_place_wave(deal_here, g, key, seed, offset, i, cur_ep + 1, mix);
        if (renew) { cur_ep++; consumed = 1; seats_dirty = true; }
    }
    if (valid) {
        TK_STREAM_STORE(&obs[i], obs_word(g, fin));
        if (done) TK_STREAM_STORE(&done[i], (uint8_t)(fin ? 1 : 0));
    }
    // ---- state back; the refill list of this launch (see play_role).  LAZY: the one line a slot emptied by taking its next
    // game goes on the group's stretch list instead (refill_role: dealt in bulk, up to TK_BULK_EVERY launches later; nothing
    // of this slot is re-dealt during the next launch, so `cprev` stays 0); only a slot that dealt a game in place lists
    // its fourteen lines for the next launch, as play_role does
    const u32 np = resync ? (u32)TK_AHEAD : (lazy ? 0u : consumed);
    if (valid) {
        g.cprev = np;                        // the next launch must not read those lines
        if (consumed) { cnt[i].episode = cur_ep; gkey[i] = key; }
        if (res != -2 || consumed || cprev0 != np) store_game(g, s01, s23, i, seats_dirty || cprev0 != np);
    }
    if (valid && np) {
        u32 p0 = atomicAdd(&push_count, np);
        push_ep[tid] = cur_ep;
        for (u32 j = 0; j < np; j++) push_list[p0 + j] = (unsigned short)(j * TK_BLOCK + tid);
    }
    if (lazy && valid && consumed && !resync) late_list[atomicAdd(&late_count, 1u)] = ((u64)(cur_ep + TK_AHEAD) << 32) | tid;
    __syncthreads();
    // ---- the games that ended with this card, scored one per lane: final_scores from the final state alone
    // (Klop.py:36-45, Berac.py:33-44, Navadna_igra.py:80-113); reward row and score sums of the slot
    if (active)
        for (u32 e = tid, nf = fin_count; e < nf; e += TK_BLOCK) {
            Game f;
            f.A = TK_U64(finq[0][e], finq[1][e]); f.B = TK_U64(finq[2][e], finq[3][e]); f.C = TK_U64(finq[4][e], finq[5][e]);
            u32 m = finq[7][e], t = finq[8][e];
            f.talon = TK_U64(finq[6][e], (m >> 24) & 15u);
            f.contract = m & 15; f.declarer = (m >> 4) & 3; f.king = (m >> 6) & 3; f.team = (m >> 8) & 15;
            f.tl = (m >> 12) & 7; f.trick_no = (m >> 16) & 15; f.leader = (m >> 20) & 3;
            f.trick = 0; f.nt = 0; f.phase = TK_PHASE_DONE; f.error = 0; f.epar = 0; f.cprev = 0;
            u64 sc = final_scores(f);
            int64_t it = (int64_t)group * TK_BLOCK + t;
            if (reward) {
                u64 rs = sc;
                if ((flags & TAROK_REWARD_REF) && (f.contract == TK_BERAC || f.contract == TK_ODPRTI_BERAC)) {
                    // what rezultat_igre folds into a Berac defender's last transition (Igralec.py:434-437):
                    // -20 when the hands are empty at the end (all twelve tricks were played), else +20
                    int dv = f.trick_no >= 12 ? -20 : 20;
                    u32 d = f.declarer;
                    rs = pack_scores(d == 0 ? (int)(int16_t)(sc & 0xFFFF) : dv, d == 1 ? (int)(int16_t)((sc >> 16) & 0xFFFF) : dv,
                                     d == 2 ? (int)(int16_t)((sc >> 32) & 0xFFFF) : dv, d == 3 ? (int)(int16_t)(sc >> 48) : dv);
                }
                reinterpret_cast<u64 *>(reward)[it] = rs;
            }
            cnt[it].score_sum = make_int4((int)finq[9][e] + (int16_t)(sc & 0xFFFF), (int)finq[10][e] + (int16_t)((sc >> 16) & 0xFFFF),
                                          (int)finq[11][e] + (int16_t)((sc >> 32) & 0xFFFF), (int)finq[12][e] + (int16_t)(sc >> 48));
        }
    // ---- the lists: nothing to write in most launches (the refill roles clear the lengths they have worked off), and then
    // the launch's number is not even worked out
    const u32 total = push_count, late = lazy ? late_count : 0u;
    if ((total | late) == 0) return;
    const u32 phase = launch_phase<LAZY ? 0 : 1>(count, play_groups, fan), par = phase & 1u;    // (`count` was requested before the state: it arrived with it)
    if (total) {
        u64 *lst = rlist + ((int64_t)group * 2 + par) * TK_REFILL_CAP;
        if (active)
            for (u32 j = tid; j < total; j += TK_BLOCK) {          // list entry: episode to deal << 32 | slot in group
                u32 en = push_list[j], t = en % TK_BLOCK;
                lst[j] = ((u64)(push_ep[t] + TK_AHEAD - en / TK_BLOCK) << 32) | t;
            }
        if (tid == 0) rcount[TK_RC(group, par)] = total;
    }
    if (lazy && late) {
        const u32 eb = (phase / TK_BULK_EVERY) & 1u;       // this stretch's list; entries beyond its capacity are dropped (never:
        const u32 fill = eb ? efill1 : efill0;             // a slot ends at most four games in a stretch; a dropped line would
        u64 *el = elist + ((int64_t)group * 2 + eb) * TK_BULK_CAP;          // just stay stale)
        if (active && tid < late && fill + tid < TK_BULK_CAP) el[fill + tid] = late_list[tid];
        if (tid == 0) rcount[TK_RC(group, 2 + eb)] = min(fill + late, (u32)TK_BULK_CAP);
    }
}

// (the library is built with kernel-argument preload — the first fourteen dwords arrive in scalar registers with the
// dispatch instead of behind a scalar load: tarok_amd/_native.py.  Putting the state pointers first instead of the scalars
// measured no better at 65,536 games and 3 % worse at 262,144: profiles/r04_ab_step.txt)
#define TK_STEP_ARGS                                                                                                              \
    int64_t n, u64 seed, u64 offset, int mix, int flags, u32 play_groups, u32 *epoch, u32 fan,                                    \
        const uint8_t *__restrict__ action_in, uint8_t *__restrict__ action_out, int16_t *__restrict__ reward,                    \
        uint8_t *__restrict__ done, uint16_t *__restrict__ trick, u64 *__restrict__ obs, uint8_t *__restrict__ hist,              \
        ulonglong2 *__restrict__ s01, ulonglong2 *__restrict__ s23, Aux *aux, Counters *__restrict__ cnt,                         \
        u64 *__restrict__ gkey, u64 *rlist, u32 *rcount, u64 *elist
// The one-card kernel is compiled for four waves per SIMD: a 128-VGPR bucket, v127 its last register (TK_KERNEL /
// TK_VGPR_TOP, tarok_device.h).
// LAZY: the env deals the lines its one-card launches empty in bulk (TAROK_OPT_LAZY_REFILL, refill_role<true>); the other
// instantiation carries none of that — where the batch streams, a dozen instructions per step wave are 3 % of a launch
template <bool RANDOM, bool LAZY>
TK_KERNEL(TK_BLOCK, 128) __attribute__((amdgpu_waves_per_eu(4))) void k_step(TK_STEP_ARGS) {
    TK_VGPR_TOP(128, 127);
    TkCount count = launch_count<LAZY ? 0 : 1>(epoch, play_groups);
    __shared__ u32 finq[FINQ_WORDS][TK_BLOCK];
    if (LAZY) {
        // Kind 0 (launch_count): one workgroup per group and nothing else.  It plays the group's card, then works the
        // group's own lists off: the per-launch list of the previous launch (only slots that dealt a game in place list
        // anything there: empty in nearly every launch) and, in the first launch of a stretch, the previous stretch's
        // list — every workgroup one pass of the deal on ~100-200 lanes.  (Round 3 had 256 refill workgroups beside the
        // 256 step workgroups at 65,536 games; with nothing to do in fifteen launches of sixteen they still cost every
        // launch ~0.9 us of dispatch and wave slots: profiles/r04_ab_step.txt.)
        step_role<RANDOM, true>(blockIdx.x, threadIdx.x, true, 255u, true, n, seed, offset, mix, flags, count, epoch, play_groups, fan, action_in,
                                action_out, reward, done, trick, obs, hist, s01, s23, aux, cnt, gkey, rlist, rcount, elist, finq);
        refill_role<true>(blockIdx.x, threadIdx.x, TK_BLOCK, seed, offset, mix, play_groups, count, epoch, fan, true, aux, rlist, rcount, elist);
    } else {
        // Kind 1, the streaming batches: the refill workgroups are spread among the play workgroups — block q (fan + 1)
        // works the lists of the `fan` play groups in the blocks after it off — so that their deals (instruction bound,
        // ~2.7k per game) run UNDER the play workgroups' streaming instead of after it: at the end of the grid they were a
        // 24 us tail of every launch that follows a trick's last card at 4 M games (profiles/r03_step_durations.txt).
        u32 q = blockIdx.x / (fan + 1), r = blockIdx.x % (fan + 1);
        if (r == 0)
            refill_role<false>(q, threadIdx.x, TK_BLOCK, seed, offset, mix, play_groups, count, epoch, fan, false, aux, rlist, rcount, elist);
        else
            step_role<RANDOM, false>(blockIdx.x - q - 1, threadIdx.x, true, 255u, false, n, seed, offset, mix, flags, count, epoch, play_groups, fan,
                                     action_in, action_out, reward, done, trick, obs, hist, s01, s23, aux, cnt, gkey, rlist, rcount, elist, finq);
    }
}

// Whole games in registers: deal, setup, Bot exchange, random play to the end.
TK_KERNEL(TK_BLOCK, 96) void k_rollout(int64_t n, u64 seed, u64 offset, u32 episode, int mix,
                                                     int16_t *__restrict__ scores_out, int16_t *__restrict__ nsteps_out,
                                                     int8_t *__restrict__ seats, u64 *__restrict__ masks,
                                                     uint8_t *__restrict__ actions) {
    TK_VGPR_TOP(96, 95);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 key = game_key(seed, offset + (u64)i, episode);
    u64 h0, h1, h2, h3, tal;
    deal_thread(key, h0, h1, h2, h3, tal);
    u32 c, d, k;
    sample_setup(key, mix, c, d, k);
    Game g;
    setup_game(g, h0, h1, h2, h3, tal, c, d, k);
    if (g.phase == TK_PHASE_EXCHANGE) bot_exchange(g, key);
    u64 scores = 0;
    int played = 0;
    // one card; NT = its position in the trick, a compile-time constant (every lane starts its game
    // at a trick boundary and plays one card per step): see play_role's trick-aligned loop
    auto card = [&](auto nt_tag, int t) __attribute__((always_inline)) {
        constexpr int NT = decltype(nt_tag)::value;
        bool live = g.phase == TK_PHASE_PLAY;
        u64 m = 0;
        u32 a = 255;
        int seat = -1;
        if (live) {
            g.nt = (u32)NT;
            m = legal_now(g);
            seat = (int)((g.leader + g.nt) & 3);
            a = policy_action(key, (u32)t, m);
            u32 ti;
            apply_step<true>(g, a, scores, ti);
            played++;
        }
        if (seats) seats[(int64_t)t * n + i] = (int8_t)seat;
        if (masks) masks[(int64_t)t * n + i] = m;
        if (actions) actions[(int64_t)t * n + i] = (uint8_t)a;
    };
    for (int t = 0; t < 48; t += 4) {
        card(std::integral_constant<int, 0>{}, t);
        card(std::integral_constant<int, 1>{}, t + 1);
        card(std::integral_constant<int, 2>{}, t + 2);
        card(std::integral_constant<int, 3>{}, t + 3);
    }
    if (scores_out) reinterpret_cast<u64 *>(scores_out)[i] = scores;
    if (nsteps_out) nsteps_out[i] = (int16_t)played;
}

// One playout, shared by every playout kernel: card c on the position h (`played` cards into its game), then the
// Bot's cards to the end under pkey (draw 128 + q at q cards played).  Returns the four final scores, packed.
__device__ __forceinline__ u64 playout_from(Game &h, u32 c, u64 pkey, u32 played) {
    u64 scores = 0;
    u32 ti, q = played + 1;
    int fin = apply_step<true>(h, c, scores, ti, false);
    // the rest of the trick the position stands in: its place in the trick is a run-time value
    while (!fin && h.nt != 0) {
        u32 card = policy_action(pkey, q, legal_now(h));
        fin = apply_step<true>(h, card, scores, ti, false);
        q++;
    }
    // whole tricks from the boundary on: the place in the trick is a compile-time constant (k_rollout)
    auto one = [&](auto nt_tag) __attribute__((always_inline)) {
        h.nt = (u32)decltype(nt_tag)::value;
        u32 card = policy_action(pkey, q, legal_now(h));
        q++;
        return apply_step<true>(h, card, scores, ti, false);
    };
    while (!fin) {
        one(std::integral_constant<int, 0>{});
        one(std::integral_constant<int, 1>{});
        one(std::integral_constant<int, 2>{});
        fin = one(std::integral_constant<int, 3>{});
    }
    return scores;
}

// ---- The playout launches (k_playout, _det, _voids, _hidden, _exchange, _bids): their shared pieces ----
#define TK_PO_MIN_LG 2
#define TK_PO_MAX_LG 8
#define TK_PO_WORLD_SLOTS 64

// A team of 2^lg lanes (4 .. 256, the host picks lg from the playouts per row) owns game g; a workgroup holds `teams` of
// them.  With worlds, the team's world records are slots slot0 .. slot0 + worlds - 1 of the workgroup's TK_PO_WORLD_SLOTS.
struct PlayoutTeam {
    u32 team, L, lane, teams;
    int64_t g;
    u32 slot0;
    __device__ __forceinline__ PlayoutTeam(u32 lg, u32 worlds = 0)
        : team(threadIdx.x >> lg), L(1u << lg), lane(threadIdx.x & (L - 1u)), teams((u32)TK_BLOCK >> lg),
          g((int64_t)blockIdx.x * teams + team), slot0(team * worlds) {}
    // zeroes the workgroup's row blocks of INTS sums per team (no barrier: the caller's next one covers it) -> the team's block
    template <u32 INTS> __device__ __forceinline__ int *zero_rows(int *sums) const {
        for (u32 w = threadIdx.x; w < teams * INTS; w += TK_BLOCK) sums[w] = 0;
        return sums + team * INTS;
    }
};

// The four scores of one playout into row j of a team's block: integer LDS adds, so the sums do not depend on the lane layout.
__device__ __forceinline__ void add_scores(int *row, u32 j, u64 scores) {
    atomicAdd(row + j * 4 + 0, (int)(int16_t)scores);
    atomicAdd(row + j * 4 + 1, (int)(int16_t)(scores >> 16));
    atomicAdd(row + j * 4 + 2, (int)(int16_t)(scores >> 32));
    atomicAdd(row + j * 4 + 3, (int)(int16_t)(scores >> 48));
}

// The smallest of rows 0 .. count - 1 at the maximum of `seat`'s sums.
__device__ __forceinline__ u32 best_row(const int *row, u32 count, u32 seat) {
    u32 best = 0;
    int top = row[seat];
    for (u32 j = 1; j < count; j++) {
        int v = row[j * 4 + seat];
        if (v > top) { top = v; best = j; }
    }
    return best;
}

// The position a card launch plays from.  All zero for a game that is not in play.
struct CardPosition {
    u64 legal = 0;
    u32 mover = 0, played = 0;
    bool in_play = false, takes_part = false;        // takes_part: in play with the mover in the game's seat set
};
__device__ __forceinline__ CardPosition card_position(const Game &g0, const uint8_t *__restrict__ seat_sets, u32 seats, int64_t g) {
    CardPosition p;
    p.in_play = g0.phase == TK_PHASE_PLAY;
    if (p.in_play) {
        p.legal = legal_now(g0);
        p.mover = (g0.leader + g0.nt) & 3;
        p.played = g0.trick_no * 4 + g0.nt;
        u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
        p.takes_part = (set >> p.mover) & 1u;
    }
    return p;
}

// A card launch's outputs for game t.g (t.g < n): the team's twelve 16-byte rows, and on lane 0 the card — the smallest
// rank at the maximum of the mover's sums, the Bot's card where the mover is outside the seat set, 255 where nothing is
// to be played.
__device__ __forceinline__ void card_epilogue(const PlayoutTeam &t, const int *row, const CardPosition &p, u32 nlegal,
                                              const u64 *__restrict__ gkey, int4 *__restrict__ sum_out, uint8_t *__restrict__ action_out) {
    if (sum_out)
        for (u32 r = t.lane; r < TAROK_PLAYOUT_RANKS; r += t.L) sum_out[t.g * TAROK_PLAYOUT_RANKS + r] = reinterpret_cast<const int4 *>(row)[r];
    if (action_out && t.lane == 0) {
        u32 act = 255;
        if (p.takes_part) act = kth_bit(p.legal, best_row(row, nlegal, p.mover));
        else if (p.in_play) act = policy_action(gkey[t.g], p.played, p.legal);
        action_out[t.g] = (uint8_t)act;
    }
}

// What a dealt world leaves in LDS for the items that play in it: one record per world slot, as separate arrays.
struct WorldAB {                                     // (A plane, B plane, team), 20 bytes a world: _det, _voids, _exchange
    u64 a[TK_PO_WORLD_SLOTS], b[TK_PO_WORLD_SLOTS];
    u32 team[TK_PO_WORLD_SLOTS];
    __device__ __forceinline__ void store(u32 slot, const Game &d) { a[slot] = d.A; b[slot] = d.B; team[slot] = d.team; }
    __device__ __forceinline__ void load(u32 slot, Game &h) const { h.A = a[slot]; h.B = b[slot]; h.team = team[slot]; }
};
struct WorldABCT {                                   // (A, B, C, talon ids, team), 36 bytes a world: _hidden, whose re-deal
    u64 a[TK_PO_WORLD_SLOTS], b[TK_PO_WORLD_SLOTS], c[TK_PO_WORLD_SLOTS], ids[TK_PO_WORLD_SLOTS];   // moves C-plane and talon cards
    u32 team[TK_PO_WORLD_SLOTS];
    __device__ __forceinline__ void store(u32 slot, const Game &d) {
        a[slot] = d.A; b[slot] = d.B; c[slot] = d.C; ids[slot] = d.talon; team[slot] = d.team;
    }
    __device__ __forceinline__ void load(u32 slot, Game &h) const {
        h.A = a[slot]; h.B = b[slot]; h.C = c[slot]; h.talon = ids[slot]; h.team = team[slot];
    }
};
struct NoWorlds {                                    // the open-hand launch: the position itself is the one world
    __device__ __forceinline__ void store(u32, const Game &) {}
    __device__ __forceinline__ void load(u32, Game &) const {}
};

// The dealers of the card launches: which worlds the playouts run in.  Extra is the dealer's per-game word (NoWord: none),
// deal() turns a copy of the position into world `key`'s, and the tags are the top bits of the game_key counters.
struct NoWord {};
template <class T> __device__ __forceinline__ T game_word(const T *__restrict__ words, int64_t g) {
    if constexpr (std::is_empty<T>::value) return T{}; else return words[g];
}
struct DealOpen {                                    // k_playout: the true hands
    static constexpr bool has_worlds = false;
    using Record = NoWorlds;
    using Extra = NoWord;
    static constexpr u64 world_tag = 0, item_tag = 1ULL << 63;
    __device__ static __forceinline__ void deal(Game &, u32, u64, NoWord) {}
};
template <class R, class X> struct DealWorlds {
    static constexpr bool has_worlds = true;
    using Record = R;
    using Extra = X;
    static constexpr u64 world_tag = 7ULL << 61, item_tag = 3ULL << 62;
};
struct DealUnseen : DealWorlds<WorldAB, NoWord> {    // k_playout_det: the cards the mover cannot see, re-dealt
    __device__ static __forceinline__ void deal(Game &d, u32 mover, u64 key, NoWord) { redeal_unseen(d, mover, key); }
};
struct DealVoids : DealWorlds<WorldAB, u32> {        // k_playout_voids: ... and no seat a card of a class it has shown void in
    __device__ static __forceinline__ void deal(Game &d, u32 mover, u64 key, u32 voids) { redeal_voids(d, mover, key, voids); }
};
struct DealHidden : DealWorlds<WorldABCT, u64> {     // k_playout_hidden: ... and Klop's talon and the declarer's discards too
    __device__ static __forceinline__ void deal(Game &d, u32 mover, u64 key, u64 played) { redeal_hidden(d, mover, key, played); }
};

// The card launches' one body: Monte-Carlo playouts from the env's CURRENT positions, read-only on the env.  A team owns
// one game.  With worlds, a world is dealt ONCE: lanes w = lane, lane + L, ... of the team each deal one world under the
// world key and leave its record in LDS (teams * worlds <= TK_PO_WORLD_SLOTS by the host's lg); without, the position's
// true hands are the one world.  After one barrier the game's work items (rank j of a legal card, world w, sample k),
// nlegal * worlds * samples of them, go round-robin over the team's lanes, so a follower's two legal cards keep as many
// lanes busy as a leader's twelve: each unpacks the position, loads its world and runs playout_from under the item key.
// All lanes of a team play the same game on from the same card count: their playouts have the same length (a Berac may
// end early in some of them), and the loops branch on team-uniform values.  The four scores go into the team's [12][4]
// row block in LDS; after a second barrier card_epilogue writes the rows and the card.  A game that does not take part
// runs no playout: zero rows.  Nothing of the env is written; no global atomics.
template <class Dealer>
__device__ __forceinline__ void playout_cards_body(int64_t n, u64 pseed, u64 offset, u32 worlds, u32 samples, u32 lg, u32 seats,
                                                   const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                                   const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,
                                                   const u64 *__restrict__ gkey, const typename Dealer::Extra *__restrict__ extra,
                                                   int4 *__restrict__ sum_out, uint8_t *__restrict__ action_out) {
    __shared__ __attribute__((aligned(16))) int sums[(TK_BLOCK >> TK_PO_MIN_LG) * TAROK_PLAYOUT_RANKS * 4];
    __shared__ typename Dealer::Record world;
    const PlayoutTeam t(lg, worlds);
    const int64_t g = t.g;
    int *row = t.zero_rows<TAROK_PLAYOUT_RANKS * 4>(sums);
    ulonglong2 a = {0, 0}, b = {0, 0};
    CardPosition p;
    u64 ebase = 0;
    u32 nlegal = 0;
    if (g < n) {
        a = s01[g]; b = s23[g];
        Game g0;
        unpack(g0, a.x, a.y, b.x, b.y);
        p = card_position(g0, seat_sets, seats, g);
        if (p.takes_part) {
            nlegal = (u32)popc64(p.legal);
            ebase = ((u64)cnt[g].episode << 28) | ((u64)p.played << 22);
            if constexpr (Dealer::has_worlds) {
                const typename Dealer::Extra word = game_word(extra, g);
                for (u32 w = t.lane; w < worlds; w += t.L) {
                    Game d = g0;
                    Dealer::deal(d, p.mover, game_key(pseed, offset + (u64)g, Dealer::world_tag | ebase | (u64)w), word);
                    world.store(t.slot0 + w, d);
                }
            }
        }
    }
    __syncthreads();
    if (p.takes_part) {
        const u32 per_card = Dealer::has_worlds ? worlds * samples : samples, items = nlegal * per_card;
        for (u32 i = t.lane; i < items; i += t.L) {
            u32 j = i / per_card, k = i - j * per_card, w = 0;
            if constexpr (Dealer::has_worlds) { w = k / samples; k -= w * samples; }
            u32 c = kth_bit(p.legal, j);
            u64 pkey = game_key(pseed, offset + (u64)g, Dealer::item_tag | ebase | ((u64)c << 16) | ((u64)w << 10) | (u64)k);
            Game h;
            unpack(h, a.x, a.y, b.x, b.y);
            world.load(t.slot0 + w, h);
            add_scores(row, j, playout_from(h, c, pkey, p.played));
        }
    }
    __syncthreads();
    if (g < n) card_epilogue(t, row, p, nlegal, gkey, sum_out, action_out);
}

// tarok_playout_cards: the open-hand launch — the playouts see the true hidden hands (perfect information, not a fair player).
TK_KERNEL(TK_BLOCK, 128) void k_playout(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 samples, u32 lg, u32 seats,
                                       const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                       const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,
                                       const u64 *__restrict__ gkey, int4 *__restrict__ sum_out, uint8_t *__restrict__ action_out) {
    TK_VGPR_TOP(128, 127);
    playout_cards_body<DealOpen>(n, pseed, offset, 0u, samples, lg, seats, seat_sets, s01, s23, cnt, gkey, nullptr, sum_out, action_out);
}

// tarok_playout_cards_det: determinized playouts — k_playout's sibling for a FAIR player.  The playouts of world w run on
// a re-deal of the cards the mover cannot see (redeal_unseen under the world key), so the result is a function of the
// mover's information set alone.
TK_KERNEL(TK_BLOCK, 128) void k_playout_det(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 worlds, u32 samples, u32 lg,
                                           u32 seats, const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                           const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,
                                           const u64 *__restrict__ gkey, int4 *__restrict__ sum_out, uint8_t *__restrict__ action_out) {
    TK_VGPR_TOP(128, 127);
    playout_cards_body<DealUnseen>(n, pseed, offset, worlds, samples, lg, seats, seat_sets, s01, s23, cnt, gkey, nullptr, sum_out, action_out);
}

// tarok_playout_exchange: the declarer's talon exchange valued by determinized playouts — k_playout_det's structure one
// decision earlier.  A team of 2^lg lanes owns one game that waits for the exchange (lg >= TK_PX_MIN_LG, by k_playout's
// rule on worlds * samples, so teams <= 16 and teams * worlds <= TK_PO_WORLD_SLOTS).  The viewer of every world is the
// DECLARER: redeal_unseen runs on the game as it waits — plane C holds the whole talon there, so no talon card is in a
// hand, the pool is the three other hands, and a new team re-parks all six talon cards; apply_exchange afterwards moves
// the chosen group to the declarer and leaves the rest where the world parked it.  Dealing lanes leave (A, B, team) of
// each world in LDS and the packed discards of each candidate (group i, set d) beside them; after ONE barrier the items
// (i, d, w, k), ngroups * sets * worlds * samples of them, go round-robin over the team: unpack, the world's planes, the
// candidate's exchange, the Bot's first card, playout_from.  Sums go into the team's [48][4] rows by integer LDS adds; a
// last pass writes 6 * sets 16-byte rows and lane 0 scans for the choice.  Nothing of the env is written; no global atomics.
#define TK_PX_MIN_LG 4
#define TK_PX_ROWS 48                                // 6 groups x 8 discard sets
TK_KERNEL(TK_BLOCK, 128) void k_playout_exchange(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 worlds, u32 samples, u32 sets,
                                                u32 lg, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                                const Counters *__restrict__ cnt, const u64 *__restrict__ gkey,
                                                int4 *__restrict__ sum_out, int8_t *__restrict__ choice_out,
                                                uint8_t *__restrict__ discards_out) {
    TK_VGPR_TOP(128, 127);
    __shared__ __attribute__((aligned(16))) int sums[(TK_BLOCK >> TK_PX_MIN_LG) * TK_PX_ROWS * 4];
    __shared__ WorldAB world;
    __shared__ u32 cand_dpk[(TK_BLOCK >> TK_PX_MIN_LG) * TK_PX_ROWS];
    const PlayoutTeam t(lg, worlds);
    const u32 L = t.L, lane = t.lane;
    const int64_t g = t.g;
    int *row = t.zero_rows<TK_PX_ROWS * 4>(sums);
    u32 *cand = cand_dpk + t.team * TK_PX_ROWS;
    ulonglong2 a = {0, 0}, b = {0, 0};
    u64 ebase = 0;
    u32 declarer = 0, ncand = 0;
    bool waiting = false, takes_part = false;
    if (g < n) {
        a = s01[g]; b = s23[g];
        Game g0;
        unpack(g0, a.x, a.y, b.x, b.y);
        waiting = g0.phase == TK_PHASE_EXCHANGE;
        declarer = g0.declarer;
        if (waiting) {
            u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
            takes_part = (set >> declarer) & 1u;
        }
        if (takes_part) {
            const u32 gs = group_size(g0.contract);
            ncand = (gs == 3 ? 2u : (gs == 2 ? 3u : 6u)) * sets;
            ebase = (u64)cnt[g].episode << 28;
            for (u32 w = lane; w < worlds; w += L) {
                Game d = g0;
                redeal_unseen(d, declarer, game_key(pseed, offset + (u64)g, (7ULL << 61) | ebase | (63ULL << 22) | (u64)w));
                world.store(t.slot0 + w, d);
            }
            for (u32 r = lane; r < ncand; r += L) {
                u32 i = r / sets, d = r - i * sets;
                cand[r] = exchange_discards(g0, i, game_key(pseed, offset + (u64)g, (5ULL << 61) | ebase | ((u64)i << 6) | (u64)d));
            }
        }
    }
    __syncthreads();
    if (takes_part) {
        const u32 per_cand = worlds * samples, items = ncand * per_cand;
        for (u32 it = lane; it < items; it += L) {
            u32 r = it / per_cand, rem = it - r * per_cand, w = rem / samples, k = rem - w * samples;
            u32 i = r / sets, d = r - i * sets;
            u64 pkey = game_key(pseed, offset + (u64)g,
                                (3ULL << 62) | ebase | (63ULL << 22) | ((u64)(8u * i + d) << 16) | ((u64)w << 10) | (u64)k);
            Game h;
            unpack(h, a.x, a.y, b.x, b.y);
            world.load(t.slot0 + w, h);
            const u32 dpk = cand[r];
            apply_exchange(h, i, dpk & 255, (dpk >> 8) & 255, (dpk >> 16) & 255);
            u32 c = policy_action(pkey, 0u, legal_now(h));
            add_scores(row, r, playout_from(h, c, pkey, 0u));
        }
    }
    __syncthreads();
    if (g >= n) return;
    const u32 nrows = 6u * sets;                     // rows at or beyond ncand stay zero: groups the contract does not have
    if (sum_out)
        for (u32 r = lane; r < nrows; r += L) sum_out[g * nrows + r] = reinterpret_cast<const int4 *>(row)[r];
    if ((choice_out || discards_out) && lane == 0) {
        int ch = -1;
        u32 dpk = 0xFFFFFFu;
        if (takes_part) {                            // the first candidate at the maximum of the declarer's sums
            const u32 best = best_row(row, ncand, declarer);
            ch = (int)(best / sets);
            dpk = cand[best];
        } else if (waiting) {                        // the Bot's own exchange: group 0, its sampler under the game's key
            Game g0;
            unpack(g0, a.x, a.y, b.x, b.y);
            ch = 0;
            dpk = exchange_discards(g0, 0u, gkey[g]);
        }
        if (choice_out) choice_out[g] = (int8_t)ch;
        if (discards_out) {
            discards_out[g * 3 + 0] = (uint8_t)dpk; discards_out[g * 3 + 1] = (uint8_t)(dpk >> 8);
            discards_out[g * 3 + 2] = (uint8_t)(dpk >> 16);
        }
    }
}

// tarok_shown_voids: the voids the play of every game has shown so far, one word per game (bit 5 * seat + class).  One lane
// per game: the history bytes 0 .. played - 1 (nothing at or beyond `played` is read: those entries are stale), the trick
// leaders replayed from the cards (first_leader / next_leader, as k_observe_ref does), and per follower card of another
// class than the card led: void in the class led, and void in taroks too when neither card is a tarok (Navadna_igra.py:
// 158-168: suit, else tarok, else anything).  Read-only; every row written, 0 for a game that is not in play.
TK_KERNEL(TK_BLOCK, 64) void k_shown_voids(int64_t n, const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                          const uint8_t *__restrict__ hist, u32 *__restrict__ voids_out) {
    TK_VGPR_TOP(64, 63);
    const int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    Game g;
    load_game(g, s01, s23, i);
    const u32 plays = g.phase == TK_PHASE_PLAY ? g.trick_no * 4 + g.nt : 0u;
    u32 lead = first_leader(g.contract, g.declarer), v = 0;
    for (u32 t = 0; t < 12; t++) {
        if (t * 4 + 1 >= plays) break;                                    // a trick shows nothing before its second card
        u32 c[4];
#pragma unroll
        for (u32 j = 0; j < 4; j++) {
            const u32 idx = t * 4 + j;
            const bool has = idx < plays;
            c[j] = has ? (u32)hist[(int64_t)idx * n + i] & 63u : 0u;
            const u32 L = min(c[0] >> 3, 4u), K = min(c[j] >> 3, 4u), seat = (lead + j) & 3;
            const bool off = has && j > 0 && K != L;
            u32 m = (1u << L) | ((K != 4 && L != 4) ? 16u : 0u);
            v |= off ? m << (5 * seat) : 0u;
        }
        if (t * 4 + 4 <= plays) lead = next_leader(lead, c);
    }
    voids_out[i] = v;
}

// tarok_playout_cards_voids: k_playout_det with worlds that honour shown voids — world w is redeal_voids(..., voids[g])
// under the same world key; a game whose word shows no void of another seat gets redeal_unseen's worlds.  The binomials come
// from constant memory (tk_binom); the (a, b) weights are recomputed per world in registers, so the LDS is k_playout_det's.
TK_KERNEL(TK_BLOCK, 128) void k_playout_voids(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 worlds, u32 samples, u32 lg,
                                             u32 seats, const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                             const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,
                                             const u64 *__restrict__ gkey, const u32 *__restrict__ voids,
                                             int4 *__restrict__ sum_out, uint8_t *__restrict__ action_out) {
    TK_VGPR_TOP(128, 127);
    playout_cards_body<DealVoids>(n, pseed, offset, worlds, samples, lg, seats, seat_sets, s01, s23, cnt, gkey, voids, sum_out, action_out);
}

// tarok_played_cards: the cards of every game's play history as one word per game (bit c: card c has been played, the
// cards on the table included).  One lane per game: the history bytes 0 .. played - 1 (those at or beyond `played` are
// stale and are not read).  The packed state cannot tell the declarer's discards from the declarer's won tricks — both
// are C-plane bits with the declarer's owner bits; pile_of(declarer) & ~word are the discards.  Read-only; every row
// written, 0 for a game that waits for the exchange.
TK_KERNEL(TK_BLOCK, 64) void k_played_cards(int64_t n, const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                           const uint8_t *__restrict__ hist, u64 *__restrict__ played_out) {
    TK_VGPR_TOP(64, 63);
    const int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    Game g;
    load_game(g, s01, s23, i);
    const u32 plays = g.phase >= TK_PHASE_PLAY ? min(g.trick_no * 4 + g.nt, 48u) : 0u;
    u64 m = 0;
    for (u32 p = 0; p < plays; p++) m |= 1ULL << ((u32)hist[(int64_t)p * n + i] & 63u);
    played_out[i] = m & TK_DECK;
}

// tarok_playout_cards_hidden: k_playout_det with worlds that also hide what only other seats have seen — Klop's face-down
// talon and the declarer's discards (redeal_hidden under the same world key; played[g] tells the discards from the won
// tricks).  A world's record is WorldABCT: the C plane changes where a discard or a talon card changes places with a hand
// card, and a Klop's gifts are read from the world's ids (apply_step).
TK_KERNEL(TK_BLOCK, 128) void k_playout_hidden(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 worlds, u32 samples, u32 lg,
                                              u32 seats, const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                              const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,
                                              const u64 *__restrict__ gkey, const u64 *__restrict__ played_words,
                                              int4 *__restrict__ sum_out, uint8_t *__restrict__ action_out) {
    TK_VGPR_TOP(128, 127);
    playout_cards_body<DealHidden>(n, pseed, offset, worlds, samples, lg, seats, seat_sets, s01, s23, cnt, gkey, played_words, sum_out, action_out);
}

// tarok_playout_cards_halving: the card launches with sequential halving — playout_cards_body's team, dealers, keys and
// playout_from, with a round loop around the item walk.  `ends`: the cumulative world counts e_0 .. e_{rounds-1}, a byte
// each (e <= 64); the team deals all e_{rounds-1} worlds once.  Round r walks (ranks alive) x (worlds e_{r-1} .. e_r - 1) x
// samples items round-robin over the team's lanes; after the barrier every lane of the team reads the team's rows and
// computes the same new `alive` word (halve_alive), and a second barrier keeps a team of several waves from adding the
// next round's scores to a row another of its waves still reads.  `ends` is launch-uniform, so every lane of the
// workgroup meets the same 2 * rounds barriers whether or not its game still plays.  A team's block in LDS is its [12][4] sums and
// behind them its twelve counts (48 bytes a team): after a round the ranks that played it get samples x the round's end.
// No global traffic between the rounds, nothing of the env written.
template <class Dealer>
__device__ __forceinline__ void playout_halving_body(int64_t n, u64 pseed, u64 offset, u32 ends, u32 samples, u32 lg, u32 seats,
                                                     const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                                     const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,
                                                     const u64 *__restrict__ gkey, const typename Dealer::Extra *__restrict__ extra,
                                                     int4 *__restrict__ sum_out, int4 *__restrict__ count_out, uint8_t *__restrict__ action_out) {
    static_assert(Dealer::has_worlds, "halving runs in dealt worlds");
    constexpr u32 INTS = TAROK_PLAYOUT_RANKS * 5;       // a team's block: [12][4] sums, [12] counts
    __shared__ __attribute__((aligned(16))) int sums[(TK_BLOCK >> TK_PO_MIN_LG) * INTS];
    __shared__ typename Dealer::Record world;
    // what only the epilogue needs waits in LDS — the launch's pointers and a flag byte per team (1: in play, 2: takes part):
    // the item loop runs at the scalar registers' limit, and pointers and lane masks held across the rounds would spill
    struct Epilogue { int4 *sum, *count; uint8_t *action; const u64 *gkey; int64_t n; };
    __shared__ Epilogue epilogue;
    __shared__ uint8_t flags[TK_BLOCK >> TK_PO_MIN_LG];
    if (threadIdx.x == 0) epilogue = {sum_out, count_out, action_out, gkey, n};
    const u32 worlds = ends >> 24 ? ends >> 24 : ends >> 16 ? ends >> 16 : ends >> 8 ? ends >> 8 : ends;      // the last round's end
    const PlayoutTeam t(lg, worlds);
    const int64_t g = t.g;
    int *row = t.zero_rows<INTS>(sums);
    ulonglong2 a = {0, 0}, b = {0, 0};
    CardPosition p;
    u64 ebase = 0;
    u32 alive = 0;
    if (g < n) {
        a = s01[g]; b = s23[g];
        Game g0;
        unpack(g0, a.x, a.y, b.x, b.y);
        p = card_position(g0, seat_sets, seats, g);
        if (p.takes_part) {
            alive = (1u << (u32)popc64(p.legal)) - 1u;
            ebase = ((u64)cnt[g].episode << 28) | ((u64)p.played << 22);
            const typename Dealer::Extra word = game_word(extra, g);
            for (u32 w = t.lane; w < worlds; w += t.L) {
                Game d = g0;
                Dealer::deal(d, p.mover, game_key(pseed, offset + (u64)g, Dealer::world_tag | ebase | (u64)w), word);
                world.store(t.slot0 + w, d);
            }
        }
    }
    if (t.lane == 0) flags[t.team] = (uint8_t)((u32)p.in_play | (u32)p.takes_part << 1);
    __syncthreads();
    u32 e0 = 0;
    for (u32 rest = ends; rest; rest >>= 8) {           // one round per byte of `ends`: launch-uniform
        const u32 e1 = rest & 255u;
        const u32 on = (alive & (alive - 1u)) != 0u || e0 == 0u ? alive : 0u;      // a game with one card alive plays no further round
        for (u32 j = t.lane; j < TAROK_PLAYOUT_RANKS; j += t.L)
            if ((on >> j) & 1u) row[TAROK_PLAYOUT_RANKS * 4 + j] = (int)(e1 * samples);
        const u32 per_card = (e1 - e0) * samples, items = (u32)__popc(on) * per_card;
        for (u32 i = t.lane; i < items; i += t.L) {
            u32 q = i / per_card, s = i - q * per_card, w = s / samples;
            s -= w * samples;
            w += e0;
            const u32 j = kth_bit_word(on, 0u, q), c = kth_bit(p.legal, j);
            u64 pkey = game_key(pseed, offset + (u64)g, Dealer::item_tag | ebase | ((u64)c << 16) | ((u64)w << 10) | (u64)s);
            Game h;
            unpack(h, a.x, a.y, b.x, b.y);
            world.load(t.slot0 + w, h);
            add_scores(row, j, playout_from(h, c, pkey, p.played));
        }
        __syncthreads();
        if (rest >> 8) {                                // not the last round: the better half stays (one card stays one card)
            alive = halve_alive(row, alive, p.mover);
            __syncthreads();
        }
        e0 = e1;
    }
    const Epilogue o = epilogue;
    if (g >= o.n) return;
    if (o.sum)
        for (u32 r = t.lane; r < TAROK_PLAYOUT_RANKS; r += t.L) o.sum[g * TAROK_PLAYOUT_RANKS + r] = reinterpret_cast<const int4 *>(row)[r];
    if (o.count && t.lane < 3u) o.count[g * 3 + t.lane] = reinterpret_cast<const int4 *>(row)[TAROK_PLAYOUT_RANKS + t.lane];
    if (o.action && t.lane == 0) {
        const u32 f = flags[t.team];
        u32 act = 255;
        if (f & 2u) act = kth_bit(p.legal, best_alive(row, alive, p.mover));
        else if (f & 1u) act = policy_action(o.gkey[g], p.played, p.legal);
        o.action[g] = (uint8_t)act;
    }
}

#define TK_HALVING_KERNEL(NAME, DEALER, WORDS_T)                                                                                   \
    TK_KERNEL(TK_BLOCK, 128) void NAME(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 ends, u32 samples, u32 lg,          \
                                      u32 seats, const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,         \
                                      const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,                         \
                                      const u64 *__restrict__ gkey, const WORDS_T *__restrict__ words, int4 *__restrict__ sum_out,  \
                                      int4 *__restrict__ count_out, uint8_t *__restrict__ action_out) {                             \
        TK_VGPR_TOP(128, 127);                                                                                                      \
        playout_halving_body<DEALER>(n, pseed, offset, ends, samples, lg, seats, seat_sets, s01, s23, cnt, gkey, words, sum_out, \
                                     count_out, action_out);                                                                        \
    }
TK_HALVING_KERNEL(k_playout_halving_det, DealUnseen, NoWord)         // words: nullptr
TK_HALVING_KERNEL(k_playout_halving_voids, DealVoids, u32)
TK_HALVING_KERNEL(k_playout_halving_hidden, DealHidden, u64)
#undef TK_HALVING_KERNEL

// tarok_playout_bids, first launch: the deal tarok_reset(env, episode, deals, ...) would make, one lane per game, left as
// (h0, h1, h2, h3, talon ids) in the env's bidding buffer [5][n] — the 54-key sorting network has a kernel of its own so
// that the playout kernel keeps its registers.  A deals row that k_reset would flag leaves five zeros: no viewer, zero sums.
TK_KERNEL(TK_BLOCK, 80) void k_bid_deal(int64_t n, u64 seed, u64 offset, u32 episode, const uint8_t *__restrict__ deals,
                                       u64 *__restrict__ out) {
    TK_VGPR_TOP(80, 79);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, tal = 0;
    if (deals) {
        const uint8_t *p = deals + i * 54;
        u64 h[4] = {0, 0, 0, 0};
        u64 seen = 0;
        bool bad = false;
        for (int k = 0; k < 48; k++) { u32 c = p[k]; bad |= c >= 54; c &= 63; seen |= 1ULL << c; h[k / 12] |= 1ULL << c; }
        for (int k = 0; k < 6; k++) { u32 c = p[48 + k]; bad |= c >= 54; c &= 63; seen |= 1ULL << c; tal |= (u64)c << (6 * k); }
        bad |= seen != TK_DECK;
        h0 = bad ? 0ULL : h[0]; h1 = bad ? 0ULL : h[1]; h2 = bad ? 0ULL : h[2]; h3 = bad ? 0ULL : h[3]; tal = bad ? 0ULL : tal;
    } else {
        deal_thread(game_key(seed, offset + (u64)i, episode), h0, h1, h2, h3, tal);
    }
    out[i] = h0; out[n + i] = h1; out[2 * n + i] = h2; out[3 * n + i] = h3; out[4 * n + i] = tal;
}

// tarok_playout_bids: every bid valued by determinized playouts — k_playout_exchange's structure one decision earlier
// still.  A team of 2^lg lanes owns one game (lg >= TK_PB_MIN_LG by k_playout's rule on worlds * samples, so teams <= 16
// and teams * worlds <= TK_PO_WORLD_SLOTS).  The four viewers are taken one after the other and share the team's world
// slots: for viewer v the dealing lanes leave (A, B, talon ids) of each world in LDS (bid_world), a barrier, then the
// items (row r of the rows played, world w, sample k) go round-robin over the team: bid_game, the Bot's exchange under
// the playout key where the contract has one, the Bot's first card, playout_from.  The VIEWER's score goes into the
// team's [4][20] block by integer LDS adds; a last pass writes it as twenty 16-byte pieces.  The viewer loop's barriers
// are outside every test of the game's seat set: each workgroup passes nine.  The env's games are not read.
#define TK_PB_MIN_LG 4
TK_KERNEL(TK_BLOCK, 128) void k_playout_bids(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 episode, u32 worlds, u32 samples,
                                            u32 lg, u32 contracts, u32 seats, const uint8_t *__restrict__ seat_sets,
                                            const u64 *__restrict__ deal, int4 *__restrict__ sum_out) {
    TK_VGPR_TOP(128, 127);
    __shared__ __attribute__((aligned(16))) int sums[(TK_BLOCK >> TK_PB_MIN_LG) * 4 * TAROK_BID_ROWS];
    __shared__ u64 world_a[TK_PO_WORLD_SLOTS], world_b[TK_PO_WORLD_SLOTS], world_ids[TK_PO_WORLD_SLOTS];
    // (PlayoutTeam's fields written out: through the struct this kernel compiles to six more instructions and its 19-row
    // launch measured 0.2 % slower, outside the parent's band — DESIGN 8.3)
    const u32 tid = threadIdx.x, team = tid >> lg, L = 1u << lg, lane = tid & (L - 1u), teams = (u32)TK_BLOCK >> lg;
    const int64_t g = (int64_t)blockIdx.x * teams + team;
    for (u32 w = tid; w < teams * (4 * TAROK_BID_ROWS); w += TK_BLOCK) sums[w] = 0;
    int *row = sums + team * (4 * TAROK_BID_ROWS);
    const u32 slot0 = team * worlds;                 // the team's worlds: slots slot0 .. slot0 + worlds - 1
    u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, tal = 0;
    u32 set = 0;
    if (g < n) {
        h0 = deal[g]; h1 = deal[n + g]; h2 = deal[2 * n + g]; h3 = deal[3 * n + g]; tal = deal[4 * n + g];
        set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
        if ((h0 | h1 | h2 | h3) == 0) set = 0;       // an invalid deal row
    }
    const u32 rowmask = bid_row_mask(contracts), nrows = (u32)__popc(rowmask);
    const u32 per_row = worlds * samples, items = nrows * per_row;
    const u64 ebase = (u64)episode << 28;
#pragma unroll 1
    for (u32 v = 0; v < 4; v++) {
        const bool part = (set >> v) & 1u;
        __syncthreads();                             // the rows are zero; the last viewer's items have read their worlds
        if (part) {
            for (u32 w = lane; w < worlds; w += L) {
                u64 A, B, ids;
                bid_world(h0, h1, h2, h3, tal, v, game_key(pseed, offset + (u64)g, (2ULL << 61) | ebase | ((u64)v << 6) | (u64)w), A, B, ids);
                world_a[slot0 + w] = A; world_b[slot0 + w] = B; world_ids[slot0 + w] = ids;
            }
        }
        __syncthreads();
        if (part) {
            for (u32 it = lane; it < items; it += L) {
                u32 j = it / per_row, rem = it - j * per_row, w = rem / samples, k = rem - w * samples;
                u32 r = kth_bit((u64)rowmask, j);
                u64 pkey = game_key(pseed, offset + (u64)g,
                                    (3ULL << 61) | ebase | ((u64)v << 26) | ((u64)r << 21) | ((u64)w << 15) | (u64)k);
                Game h;
                bid_game(h, world_a[slot0 + w], world_b[slot0 + w], world_ids[slot0 + w], r, v);
                if (h.phase == TK_PHASE_EXCHANGE) bot_exchange(h, pkey);
                u32 c = policy_action(pkey, 0u, legal_now(h));
                u64 scores = playout_from(h, c, pkey, 0u);
                atomicAdd(row + v * TAROK_BID_ROWS + r, (int)(int16_t)(scores >> (16 * v)));
            }
        }
    }
    __syncthreads();
    if (g >= n) return;
    for (u32 r = lane; r < TAROK_BID_ROWS; r += L) sum_out[g * TAROK_BID_ROWS + r] = reinterpret_cast<const int4 *>(row)[r];
}

// tarok_playout_bids_pass: k_playout_bids with one more kind of item per viewer, (19, w, k), the pass playout: three Bots
// bid under the item's key with the viewer muted (pass_round), the game of their contract and declarer is set up on the
// world, and the item goes on as a row's does.  Its sum is the viewer's row 19; rows 0..18 are k_playout_bids' to the byte.
// A kernel of its own, k_playout_bids' text with the item changed: as one templated body the parent's kernel compiled to
// four more instructions.  The barriers stand outside every test of the seat set as there.
TK_KERNEL(TK_BLOCK, 128) void k_playout_bids_pass(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 episode, u32 worlds, u32 samples,
                                                 u32 lg, u32 contracts, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                 const u64 *__restrict__ deal, int4 *__restrict__ sum_out) {
    TK_VGPR_TOP(128, 127);
    __shared__ __attribute__((aligned(16))) int sums[(TK_BLOCK >> TK_PB_MIN_LG) * 4 * TAROK_BID_ROWS];
    __shared__ u64 world_a[TK_PO_WORLD_SLOTS], world_b[TK_PO_WORLD_SLOTS], world_ids[TK_PO_WORLD_SLOTS];
    const u32 tid = threadIdx.x, team = tid >> lg, L = 1u << lg, lane = tid & (L - 1u), teams = (u32)TK_BLOCK >> lg;
    const int64_t g = (int64_t)blockIdx.x * teams + team;
    for (u32 w = tid; w < teams * (4 * TAROK_BID_ROWS); w += TK_BLOCK) sums[w] = 0;
    int *row = sums + team * (4 * TAROK_BID_ROWS);
    const u32 slot0 = team * worlds;                 // the team's worlds: slots slot0 .. slot0 + worlds - 1
    u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, tal = 0;
    u32 set = 0;
    if (g < n) {
        h0 = deal[g]; h1 = deal[n + g]; h2 = deal[2 * n + g]; h3 = deal[3 * n + g]; tal = deal[4 * n + g];
        set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
        if ((h0 | h1 | h2 | h3) == 0) set = 0;       // an invalid deal row
    }
    const u32 rowmask = bid_row_mask(contracts), nrows = (u32)__popc(rowmask);
    const u32 per_row = worlds * samples, items = (nrows + 1u) * per_row;
    const u64 ebase = (u64)episode << 28;
#pragma unroll 1
    for (u32 v = 0; v < 4; v++) {
        const bool part = (set >> v) & 1u;
        __syncthreads();                             // the rows are zero; the last viewer's items have read their worlds
        if (part) {
            for (u32 w = lane; w < worlds; w += L) {
                u64 A, B, ids;
                bid_world(h0, h1, h2, h3, tal, v, game_key(pseed, offset + (u64)g, (2ULL << 61) | ebase | ((u64)v << 6) | (u64)w), A, B, ids);
                world_a[slot0 + w] = A; world_b[slot0 + w] = B; world_ids[slot0 + w] = ids;
            }
        }
        __syncthreads();
        if (part) {
            for (u32 it = lane; it < items; it += L) {
                u32 j = it / per_row, rem = it - j * per_row, w = rem / samples, k = rem - w * samples;
                u32 r = j == nrows ? (u32)TK_BID_PASS_ROW : kth_bit((u64)rowmask, j);
                u64 pkey = game_key(pseed, offset + (u64)g,
                                    (3ULL << 61) | ebase | ((u64)v << 26) | ((u64)r << 21) | ((u64)w << 15) | (u64)k);
                Game h;
                // one setup for both kinds of item, so a pass item rejoins its wave's row items in front of the exchange
                u32 ct = bid_row_contract(r), d = ct == TK_KLOP ? 0u : v, kg = bid_row_king(r);
                if (r == TK_BID_PASS_ROW) pass_round(pkey, v, ct, d, kg);
                bid_game_as(h, world_a[slot0 + w], world_b[slot0 + w], world_ids[slot0 + w], ct, d, kg);
                if (h.phase == TK_PHASE_EXCHANGE) bot_exchange(h, pkey);
                u32 c = policy_action(pkey, 0u, legal_now(h));
                u64 scores = playout_from(h, c, pkey, 0u);
                atomicAdd(row + v * TAROK_BID_ROWS + r, (int)(int16_t)(scores >> (16 * v)));
            }
        }
    }
    __syncthreads();
    if (g >= n) return;
    for (u32 r = lane; r < TAROK_BID_ROWS; r += L) sum_out[g * TAROK_BID_ROWS + r] = reinterpret_cast<const int4 *>(row)[r];
}

// tarok_bid_round: one bidding round per game on one lane (bid_round, tarok_device.h): the control flow of bot_bidding
// with playout-valued answers on the seats of the set.  Every row of the three outputs is written.
TK_KERNEL(TK_BLOCK, 64) void k_bid_round(int64_t n, u64 seed, u64 offset, u32 episode, const int32_t *__restrict__ sums, int playouts,
                                        int threshold, u32 contracts, u32 seats, const uint8_t *__restrict__ seat_sets,
                                        int8_t *__restrict__ contract_out, int8_t *__restrict__ declarer_out, int8_t *__restrict__ king_out) {
    TK_VGPR_TOP(64, 63);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 set = seat_sets ? (u32)seat_sets[i] & 15u : seats;
    u32 c, d, k;
    bid_round(game_key(seed, offset + (u64)i, episode), sums + i * (4 * TAROK_BID_ROWS), playouts, threshold, contracts, set, c, d, k);
    if (contract_out) contract_out[i] = (int8_t)c;
    if (declarer_out) declarer_out[i] = (int8_t)d;
    if (king_out) king_out[i] = (int8_t)k;
}

// tarok_bid_round_pass: k_bid_round whose seats take their bar from row 19 of their own sums (bid_round's BidPassBar overload).
TK_KERNEL(TK_BLOCK, 64) void k_bid_round_pass(int64_t n, u64 seed, u64 offset, u32 episode, const int32_t *__restrict__ sums, int playouts,
                                             int margin, u32 contracts, u32 seats, const uint8_t *__restrict__ seat_sets,
                                             int8_t *__restrict__ contract_out, int8_t *__restrict__ declarer_out, int8_t *__restrict__ king_out) {
    TK_VGPR_TOP(64, 63);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 set = seat_sets ? (u32)seat_sets[i] & 15u : seats;
    u32 c, d, k;
    bid_round(game_key(seed, offset + (u64)i, episode), sums + i * (4 * TAROK_BID_ROWS), playouts, margin, contracts, set, BidPassBar{}, c, d, k);
    if (contract_out) contract_out[i] = (int8_t)c;
    if (declarer_out) declarer_out[i] = (int8_t)d;
    if (king_out) king_out[i] = (int8_t)k;
}

// tarok_playout_targets: a playout launch's sums -> one target row of 64 bf16 per game (include/tarok_env.h).  One lane per
// game builds its row in LDS — eight zero pieces, then at most twelve 2-byte values at the legal cards' columns — and the
// workgroup writes its 256 rows, 32 KB in a row of memory, as 16-byte pieces in lane order.  The mover's column of the twelve
// sums is picked by compare / select (no run-time register index), the row maximum is subtracted in integers (exact), the
// exponential is expf and the quotient a division: one float32 softmax, rounded once to bf16.
TK_KERNEL(TK_BLOCK, 128) void k_playout_targets(int64_t n, const int4 *__restrict__ sums, const u64 *__restrict__ obs, float den /* playouts * tau */,
                                              u32 seats, const uint8_t *__restrict__ seat_sets, uint4 *__restrict__ out) {
    TK_VGPR_TOP(128, 127);                          // (the twelve 16-byte loads in flight and the twelve exponentials: 80 registers)
    __shared__ __attribute__((aligned(16))) uint16_t rows[TK_BLOCK * 64];
    const u32 tid = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * TK_BLOCK, g = g0 + tid;
    uint4 *rows4 = reinterpret_cast<uint4 *>(rows);
#pragma unroll
    for (u32 i = 0; i < 8; i++) rows4[i * TK_BLOCK + tid] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    if (g < n) {
        const u64 word = obs[g], legal = word & TAROK_OBS_MASK;
        const u32 s = (u32)(word >> TAROK_OBS_SEAT_SHIFT) & 3u;
        const u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
        if (legal != 0 && ((set >> s) & 1u)) {
            u32 nl = (u32)popc64(legal);
            nl = nl < TAROK_PLAYOUT_RANKS ? nl : TAROK_PLAYOUT_RANKS;
            int v[TAROK_PLAYOUT_RANKS];
#pragma unroll
            for (u32 j = 0; j < TAROK_PLAYOUT_RANKS; j++) {
                int4 q = sums[g * TAROK_PLAYOUT_RANKS + j];
                v[j] = s == 0 ? q.x : s == 1 ? q.y : s == 2 ? q.z : q.w;
            }
            int top = v[0];
            u32 best = 0;                                // the smallest rank at the maximum: the playout launch's card
#pragma unroll
            for (u32 j = 1; j < TAROK_PLAYOUT_RANKS; j++) {
                bool up = j < nl && v[j] > top;
                top = up ? v[j] : top;
                best = up ? j : best;
            }
            float e[TAROK_PLAYOUT_RANKS], sum = 0.f;
#pragma unroll
            for (u32 j = 0; j < TAROK_PLAYOUT_RANKS; j++) {
                float x = den > 0.f ? expf((float)((int64_t)v[j] - (int64_t)top) / den) : (j == best ? 1.f : 0.f);
                e[j] = j < nl ? x : 0.f;
                sum += e[j];
            }
            u64 rest = legal;
#pragma unroll
            for (u32 j = 0; j < TAROK_PLAYOUT_RANKS; j++) {
                if (j < nl) {
                    u32 c = (u32)__builtin_ctzll(rest);
                    rest &= rest - 1;
                    rows[tid * 64 + c] = __builtin_bit_cast(uint16_t, (__bf16)(e[j] / sum));
                }
            }
        }
    }
    __syncthreads();
    const u32 pieces = (u32)(n - g0 < TK_BLOCK ? n - g0 : TK_BLOCK) * 8u;
#pragma unroll
    for (u32 i = 0; i < 8; i++) {
        u32 p = i * TK_BLOCK + tid;
        if (p < pieces) out[g0 * 8 + p] = rows4[p];
    }
}

// tarok_playout_targets_counts: k_playout_targets for sums with a count per card (a halving launch's): the same lane per
// game, LDS row and 16-byte stores.  m_j = float(sum) / float(count) is one float32 division, the maximum is taken over the
// ranks with count > 0 and a rank without playouts gets 0.  tau = 0 compares the integer sums of the ranks of maximal count
// (equal counts: comparing sums is comparing means, exactly), so on a halving launch's output it is that launch's card.
TK_KERNEL(TK_BLOCK, 128) void k_playout_targets_counts(int64_t n, const int4 *__restrict__ sums, const int4 *__restrict__ counts,
                                                     const u64 *__restrict__ obs, float tau, u32 seats,
                                                     const uint8_t *__restrict__ seat_sets, uint4 *__restrict__ out) {
    TK_VGPR_TOP(128, 127);
    __shared__ __attribute__((aligned(16))) uint16_t rows[TK_BLOCK * 64];
    const u32 tid = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * TK_BLOCK, g = g0 + tid;
    uint4 *rows4 = reinterpret_cast<uint4 *>(rows);
#pragma unroll
    for (u32 i = 0; i < 8; i++) rows4[i * TK_BLOCK + tid] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    if (g < n) {
        const u64 word = obs[g], legal = word & TAROK_OBS_MASK;
        const u32 s = (u32)(word >> TAROK_OBS_SEAT_SHIFT) & 3u;
        const u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
        if (legal != 0 && ((set >> s) & 1u)) {
            u32 nl = (u32)popc64(legal);
            nl = nl < TAROK_PLAYOUT_RANKS ? nl : TAROK_PLAYOUT_RANKS;
            int v[TAROK_PLAYOUT_RANKS], cn[TAROK_PLAYOUT_RANKS];
#pragma unroll
            for (u32 j = 0; j < TAROK_PLAYOUT_RANKS; j++) {
                int4 q = sums[g * TAROK_PLAYOUT_RANKS + j];
                v[j] = s == 0 ? q.x : s == 1 ? q.y : s == 2 ? q.z : q.w;
            }
#pragma unroll
            for (u32 j = 0; j < TAROK_PLAYOUT_RANKS / 4; j++) {
                int4 q = counts[g * (TAROK_PLAYOUT_RANKS / 4) + j];
                cn[4 * j] = q.x; cn[4 * j + 1] = q.y; cn[4 * j + 2] = q.z; cn[4 * j + 3] = q.w;
            }
            int cmax = 0;
#pragma unroll
            for (u32 j = 0; j < TAROK_PLAYOUT_RANKS; j++) {
                cn[j] = j < nl && cn[j] > 0 ? cn[j] : 0;
                cmax = cn[j] > cmax ? cn[j] : cmax;
            }
            float m[TAROK_PLAYOUT_RANKS], mtop = 0.f;
            int top = 0;
            u32 best = TAROK_PLAYOUT_RANKS, any = 0;         // best: the smallest rank at the maximal sum among the ranks of maximal count
#pragma unroll
            for (u32 j = 0; j < TAROK_PLAYOUT_RANKS; j++) {
                const bool on = cn[j] > 0;
                m[j] = on ? (float)v[j] / (float)cn[j] : 0.f;
                mtop = on && (!any || m[j] > mtop) ? m[j] : mtop;
                any |= (u32)on;
                const bool up = on && cn[j] == cmax && (best == TAROK_PLAYOUT_RANKS || v[j] > top);
                top = up ? v[j] : top;
                best = up ? j : best;
            }
            float e[TAROK_PLAYOUT_RANKS], sum = 0.f;
#pragma unroll
            for (u32 j = 0; j < TAROK_PLAYOUT_RANKS; j++) {
                float x = tau > 0.f ? expf((m[j] - mtop) / tau) : (j == best ? 1.f : 0.f);
                e[j] = cn[j] > 0 ? x : 0.f;
                sum += e[j];
            }
            u64 rest = legal;
#pragma unroll
            for (u32 j = 0; j < TAROK_PLAYOUT_RANKS; j++) {
                if (j < nl) {
                    u32 c = (u32)__builtin_ctzll(rest);
                    rest &= rest - 1;
                    if (any) rows[tid * 64 + c] = __builtin_bit_cast(uint16_t, (__bf16)(e[j] / sum));
                }
            }
        }
    }
    __syncthreads();
    const u32 pieces = (u32)(n - g0 < TK_BLOCK ? n - g0 : TK_BLOCK) * 8u;
#pragma unroll
    for (u32 i = 0; i < 8; i++) {
        u32 p = i * TK_BLOCK + tid;
        if (p < pieces) out[g0 * 8 + p] = rows4[p];
    }
}

// Observation features for the seat to move, 256 x bf16 per game (0.0 / 1.0), for a policy
// network (the feature set is the build's own: the reference's encoder belongs
// to its LSTM agent, Igralec.py:453-543).  Four 64-wide regions, each a 54-bit card set followed
// by 10 flag bits:
//   [  0, 64) own hand            | contract one-hot (10)
//   [ 64,128) legal cards (mozne) | declarer seat relative to the mover one-hot (4), cards on
//                                   the table one-hot (4), mover is on the declarer's team, Tri/Dve/Ena
//   [128,192) cards on the table  | called-king suit one-hot (4), trick number in binary (4), 0, 0
//   [192,256) cards already taken | game live, 0 ...
// The four 64-bit feature words of a game, for the seat to move (the regions above: a 54-bit card set, ten flag bits
// from bit 54): what the fused policy kernels feed their network and write to feature_words_out.
// (k_observe restates it: through this function that tuned kernel compiles to another instruction stream.)
// For a game that is not in play (waiting for the exchange, or finished) the legal region and the live bit are 0 and
// every other region is what the game's state holds (include/tarok_env.h at tarok_observe); both streams are held to
// tests/observe_model.py, the statement on the CPU oracle, by tests/test_gpu_observe_features.py.
__device__ __forceinline__ void policy_feature_words(const Game &g, u64 (&e)[4]) {
    u32 seat = (g.leader + g.nt) & 3;
    bool live = g.phase == TK_PHASE_PLAY;
    u64 on_table = 0;
    for (u32 j = 0; j < g.nt; j++) on_table |= 1ULL << ((g.trick >> (6 * j)) & 63);
    u64 f1 = (u64)(1u << ((g.declarer - seat) & 3)) | ((u64)(1u << g.nt) << 4) | ((u64)((g.team >> seat) & 1) << 8) |
             ((u64)(has_king(g.contract) ? 1u : 0u) << 9);
    u64 f2 = (has_king(g.contract) ? (u64)(1u << g.king) : 0) | ((u64)g.trick_no << 4);
    e[0] = hand_of(g, seat) | ((u64)(1u << g.contract) << 54);
    e[1] = (live ? legal_now(g) : 0) | (f1 << 54);
    e[2] = on_table | (f2 << 54);
    e[3] = (g.C & ~talon_unowned(g) & ~on_table) | ((u64)(live ? 1u : 0u) << 54);
}

// k_observe: each thread builds the four 64-bit words of its own game; then the wave writes one game per
// iteration: lane L expands bits 4L..4L+3 into 4 bf16 and the 64 lanes store one contiguous
// 512-byte row (v_readlane broadcasts the words), so the 33 MB/step of features leave as full lines.
TK_KERNEL(TK_BLOCK, 64) void k_observe(int64_t n, const ulonglong2 *__restrict__ s01,
                                                     const ulonglong2 *__restrict__ s23, uint2 *__restrict__ out) {
    TK_VGPR_TOP(64, 63);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    bool valid = i < n;
    Game g;
    load_game(g, s01, s23, valid ? i : n - 1);
    u32 seat = (g.leader + g.nt) & 3;
    bool live = g.phase == TK_PHASE_PLAY;
    u64 on_table = 0;
    for (u32 j = 0; j < g.nt; j++) on_table |= 1ULL << ((g.trick >> (6 * j)) & 63);
    u64 e0 = hand_of(g, seat) | ((u64)(1u << g.contract) << 54);
    u64 f1 = (u64)(1u << ((g.declarer - seat) & 3)) | ((u64)(1u << g.nt) << 4) | ((u64)((g.team >> seat) & 1) << 8) |
             ((u64)(has_king(g.contract) ? 1u : 0u) << 9);
    u64 e1 = (live ? legal_now(g) : 0) | (f1 << 54);
    u64 f2 = (has_king(g.contract) ? (u64)(1u << g.king) : 0) | ((u64)g.trick_no << 4);
    u64 e2 = on_table | (f2 << 54);
    u64 e3 = (g.C & ~talon_unowned(g) & ~on_table) | ((u64)(live ? 1u : 0u) << 54);
    u32 lane = __lane_id();
    u32 region = lane >> 4, shift = (lane & 15) * 4;
    int64_t wave_base = i - lane;
    for (int l = 0; l < 64; l++) {
        if (wave_base + l >= n) break;                       // wave-uniform
        u32 lo0 = (u32)__builtin_amdgcn_readlane((int)(u32)e0, l), hi0 = (u32)__builtin_amdgcn_readlane((int)(u32)(e0 >> 32), l);
        u32 lo1 = (u32)__builtin_amdgcn_readlane((int)(u32)e1, l), hi1 = (u32)__builtin_amdgcn_readlane((int)(u32)(e1 >> 32), l);
        u32 lo2 = (u32)__builtin_amdgcn_readlane((int)(u32)e2, l), hi2 = (u32)__builtin_amdgcn_readlane((int)(u32)(e2 >> 32), l);
        u32 lo3 = (u32)__builtin_amdgcn_readlane((int)(u32)e3, l), hi3 = (u32)__builtin_amdgcn_readlane((int)(u32)(e3 >> 32), l);
        u32 lo = region == 0 ? lo0 : (region == 1 ? lo1 : (region == 2 ? lo2 : lo3));
        u32 hi = region == 0 ? hi0 : (region == 1 ? hi1 : (region == 2 ? hi2 : hi3));
        u32 nib = ((shift < 32 ? lo >> shift : hi >> (shift - 32))) & 15u;
        uint2 v;
        v.x = ((nib & 1) ? 0x3F80u : 0u) | ((nib & 2) ? 0x3F800000u : 0u);
        v.y = ((nib & 4) ? 0x3F80u : 0u) | ((nib & 8) ? 0x3F800000u : 0u);
        out[(wave_base + l) * 64 + lane] = v;
    }
}

// ---------------------------------------------------------------------------
// The reference's OWN observation layout: what Nevronski_igralec builds for the
// seat to move in stanje_v_vektor_rek_navadna (Igralec.py:453-533), as one dense record of 0/1
// bytes per game (offsets TAROK_REF_* in tarok_env.h; a consumer slices views out of it):
//   opponents' history [56][3][54]  row i = the i-th card PLAYED in the game (talon entries of the
//                                   history do not take a row): one-hot card in the channel of the
//                                   opponent who played it, channels = the other seats in seat order
//                                   (igralci2index, Igralec.py:271-274)                      :508-510
//   own-hand history   [56][54]     row i of an own play = the hand vector before that card, which
//                                   starts from the hand as DEALT (zacetna_roka: the exchange is not
//                                   applied to it, discards stay set)                        :465,511-514
//   talon              [6][55]      Tri..Solo_ena: row r = one-hot of the r-th talon card, column 54 =
//                                   "in the chosen group" (:499-507); Klop: a flat 54-vector of the
//                                   talon cards gifted so far (:497-498); Berac: nothing (:487-488)
//   king one-hot [4] (:467-470), declarer-relative index one-hot [4] (:493-494, self = 3),
//   discards [54] (only in the view of the player who exchanged, :462-464), legal cards [54] (:518-519)
// plus meta = {T, network type, rows used, seat}: T = entries of the history — played cards + the
// "Talon" entry + Klop's talon gifts: the counter at :456-458 counts every entry — rounded up to the
// next multiple of 8, plus 8 when already one (:460); the reference's tensors have T rows, the
// record always 56 (rows >= rows-used are zero either way).
// Parity unpinned: the reference holds no fixture for this layout and Igralec.py cannot be imported
// (pytorch_lightning, torch_models); tested against a line-cited restatement (oracle/encoder_spec.py).
//
// Workgroup = 64 games, 256 threads.  Phase 1, one thread per game (one wave): history bytes -> LDS, trick leaders replayed from the cards (the
// winner rule of apply_step), initial hand and discards recovered from the planes, the 448 bits of
// the small fields.  Phase 2, one wave per game at a time: lane t builds row t (an exclusive
// prefix-OR over the lanes gives "own cards played before"), then the 64 lanes write the 12,544-byte
// record as 784 16-byte chunks, each computed from the row descriptors: full-line stores.
#define OR_ROWS 56
#define OR_OWN_OFF (OR_ROWS * 162)
#define OR_SMALL_OFF (OR_OWN_OFF + OR_ROWS * 54)
#define OR_REC (OR_SMALL_OFF + 448)
static_assert(OR_REC == TAROK_REF_RECORD_BYTES && OR_OWN_OFF == TAROK_REF_OWN && OR_SMALL_OFF == TAROK_REF_TALON, "record layout");

struct RefDesc { u64 h0; u64 small[7]; u32 leaders, plays, me, pad; };

// 4 bits -> 4 bytes of 0/1 (the four shifted copies do not overlap: no carries)
__device__ __forceinline__ u32 nibble_bytes(u32 x) { return ((x & 15u) * 0x00204081u) & 0x01010101u; }
__device__ __forceinline__ uint4 bits16_bytes(u32 b) {
    return make_uint4(nibble_bytes(b), nibble_bytes(b >> 4), nibble_bytes(b >> 8), nibble_bytes(b >> 12));
}
// OR `val` (WIDTH <= 64 bits) into a little-endian bit vector at the compile-time bit offset OFF
template <int OFF, int NW> __device__ __forceinline__ void bits_insert(u64 (&w)[NW], u64 val) {
    w[OFF / 64] |= val << (OFF % 64);
    if constexpr (OFF % 64 != 0 && OFF / 64 + 1 < NW) w[OFF / 64 + 1] |= val >> (64 - OFF % 64);
}
// set bit `b` (run-time index) of a bit vector kept in registers
template <int NW> __device__ __forceinline__ void bits_set(u64 (&w)[NW], u32 b) {
#pragma unroll
    for (int k = 0; k < NW; k++) w[k] |= ((b >> 6) == (u32)k) ? (1ULL << (b & 63)) : 0ULL;
}
__device__ __forceinline__ u32 ref_type(u32 c) {    // Nevronski_igralec.tip_igre_v_tip_izbire (Igralec.py:180-189), Tipi_NN values
    return c == TK_KLOP ? 0u : (has_king(c) ? 1u : ((c == TK_BERAC || c == TK_ODPRTI_BERAC) ? 3u : 2u));
}

#define OR_GAMES 64                 // games per workgroup: phase 1 on one wave, phase 2 on all four (16 games each)
TK_KERNEL(256, 64) void k_observe_ref(int64_t n, const ulonglong2 *__restrict__ s01,
                                                   const ulonglong2 *__restrict__ s23, const uint8_t *__restrict__ hist,
                                                   uint4 *__restrict__ rec, int4 *__restrict__ meta) {
    TK_VGPR_TOP(64, 63);
    __shared__ RefDesc desc[OR_GAMES];
    __shared__ uint8_t hist_s[OR_GAMES][48];
    __shared__ uint8_t rowpos_s[4][64];
    __shared__ u64 rowmask_s[4][64];
    u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t base = (int64_t)blockIdx.x * OR_GAMES;
    if (tid < OR_GAMES)
    {   // ---- phase 1
        int64_t i = base + tid;
        bool valid = i < n;
        int64_t ic = valid ? i : n - 1;
        Game g;
        load_game(g, s01, s23, ic);
        bool live = valid && g.phase == TK_PHASE_PLAY;
        u32 me = (g.leader + g.nt) & 3;
        u32 plays = live ? g.trick_no * 4 + g.nt : 0u;
        u32 lead = first_leader(g.contract, g.declarer);
        u32 leaders = 0;
        u64 played_all = 0, played_me = 0;
        for (u32 t = 0; t < 12; t++) {
            if (t * 4 >= plays) break;
            leaders |= lead << (2 * t);
            u32 c[4];
#pragma unroll
            for (u32 j = 0; j < 4; j++) {
                u32 idx = t * 4 + j;
                bool has = idx < plays;
                c[j] = has ? (u32)hist[(int64_t)idx * n + ic] & 63u : 0u;
                hist_s[tid][idx] = (uint8_t)c[j];
                u64 bit = has ? (1ULL << c[j]) : 0ULL;
                played_all |= bit;
                played_me |= (((lead + j) & 3) == me) ? bit : 0ULL;
            }
            if (t * 4 + 4 <= plays) lead = next_leader(lead, c);          // pobere_stih (Klop.py:81-94)
        }
        // zacetna_roka (Igralec.py:264): the hand as dealt.  hand now + own cards played = the hand after
        // the exchange = (dealt + chosen group) - discards; the discards are what lies in the exchanging
        // player's pile without ever having been played (Igralec.py:376-377)
        u64 h_after = hand_of(g, me) | played_me;
        u64 h0 = h_after, disc = 0;
        bool exch = has_exchange(g.contract);
        u32 gs = exch ? group_size(g.contract) : 1u;
        if (exch && me == g.declarer) {
            u64 grp = ids_mask(g.talon, (int)(g.tl * gs), (int)gs);
            disc = seat_cards(g, g.declarer) & g.C & ~played_all;
            h0 = (h_after & ~grp) | (disc & ~grp);
        }
        u64 small[7] = {0, 0, 0, 0, 0, 0, 0};
        if (live) {
            if (exch) {                                                   // the ("Talon", ...) entry, :499-507
#pragma unroll
                for (u32 r = 0; r < 6; r++) {
                    bits_set(small, r * 55 + (u32)((g.talon >> (6 * r)) & 63));
                    if (r / gs == g.tl) bits_set(small, r * 55 + 54);
                }
            } else if (g.contract == TK_KLOP) {                           // (None, talon card) entries, :497-498
#pragma unroll
                for (u32 r = 0; r < 6; r++)
                    if (r >= g.tl) bits_set(small, (u32)((g.talon >> (6 * r)) & 63));
            }
            if (has_king(g.contract)) bits_insert<330>(small, 1ULL << g.king);                       // :467-470
            u32 didx = g.declarer == me ? 3u : (g.declarer < me ? g.declarer : g.declarer - 1);     // :271-274, 449-451
            if (g.contract != TK_KLOP) bits_insert<334>(small, 1ULL << didx);                         // (Klop's list has no index, :526-527)
            bits_insert<338>(small, disc);
            bits_insert<392>(small, legal_now(g));
        }
        RefDesc &d = desc[tid];
        d.h0 = live ? h0 : 0;
#pragma unroll
        for (int k = 0; k < 7; k++) d.small[k] = small[k];
        d.leaders = leaders; d.plays = plays; d.me = me;
        if (valid && meta) {
            u32 entries = plays + (exch ? 1u : 0u) + (g.contract == TK_KLOP ? 6u - g.tl : 0u);       // :455-458
            u32 T = entries + (8 - entries % 8);                                                      // :460
            meta[i] = make_int4(live ? (int)T : 0, (int)ref_type(g.contract), (int)plays, (int)me);
        }
    }
    __syncthreads();
    // ---- phase 2: this wave's 16 games, one at a time (four waves per 64 games: at 65,536 games that is four
    // waves per SIMD to hide the stores' issue latency behind each other)
    for (u32 k = 0; k < OR_GAMES / 4; k++) {
        u32 gl = wave * (OR_GAMES / 4) + k;
        int64_t gidx = base + gl;
        if (gidx >= n) break;                                             // wave uniform
        const RefDesc &d = desc[gl];
        u32 me = d.me, plays = d.plays;
        u32 pos = 255;
        u64 mybit = 0;
        if (lane < plays) {
            u32 c = hist_s[gl][lane];
            u32 seat = (((d.leaders >> (2 * (lane >> 2))) & 3) + (lane & 3)) & 3;
            if (seat == me) mybit = 1ULL << c;
            else pos = (seat < me ? seat : seat - 1) * 54 + c;
        }
        u32 lo = (u32)mybit, hi = (u32)(mybit >> 32);                     // inclusive prefix OR over the rows
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            u32 l2 = (u32)__shfl_up((int)lo, o), h2 = (u32)__shfl_up((int)hi, o);
            if ((int)lane >= o) { lo |= l2; hi |= h2; }
        }
        u64 before = TK_U64(lo, hi) & ~mybit;                             // own cards played before this row
        rowpos_s[wave][lane] = (uint8_t)pos;
        rowmask_s[wave][lane] = mybit ? (d.h0 & ~before) : 0ULL;          // :512 (the hand before the card leaves it)
        __builtin_amdgcn_s_waitcnt(0xC07F);                               // lgkmcnt(0): the wave's LDS writes have landed
        __builtin_amdgcn_wave_barrier();
        for (u32 ch = lane; ch < OR_REC / 16; ch += 64) {
            u32 o = ch * 16;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (o < OR_OWN_OFF) {
                u32 t0 = o / 162;
#pragma unroll
                for (u32 q = 0; q < 2; q++) {
                    u32 t = t0 + q;
                    u32 pp = rowpos_s[wave][t & 63];
                    u32 idx = t * 162 + pp - o;
                    if (t < 64 && pp < 162 && idx < 16) {
                        u32 b = 1u << ((idx & 3) * 8);
                        v.x |= (idx >> 2) == 0 ? b : 0; v.y |= (idx >> 2) == 1 ? b : 0;
                        v.z |= (idx >> 2) == 2 ? b : 0; v.w |= (idx >> 2) == 3 ? b : 0;
                    }
                }
            } else if (o < OR_SMALL_OFF) {
                u32 rel = o - OR_OWN_OFF, t0 = rel / 54, b0 = rel - t0 * 54;
                u64 m = (rowmask_s[wave][t0] >> b0) | (rowmask_s[wave][(t0 + 1) & 63] << (54 - b0));
                v = bits16_bytes((u32)m & 0xFFFFu);
            } else {
                u32 rel = o - OR_SMALL_OFF;
                v = bits16_bytes((u32)(d.small[rel >> 6] >> (rel & 63)) & 0xFFFFu);
            }
            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
            u32x4 vv = {v.x, v.y, v.z, v.w};                         // (822 MB per call at 65,536 games: nothing re-reads it from L2)
            TK_STREAM_STORE(reinterpret_cast<u32x4 *>(rec) + gidx * (OR_REC / 16) + ch, vv);
        }
        __builtin_amdgcn_wave_barrier();                                  // the row buffers are rewritten by the next game
    }
}

// A block's per-game bit vectors (NW words each, in LDS) written as 0/1 bytes, BYTES per game (a multiple
// of 8), wave-cooperatively: a game's record leaves as consecutive 8-byte stores of neighbouring lanes.
template <int NW, int BYTES>
__device__ __forceinline__ void write_bit_records(const u64 (*words)[NW], int64_t base, int64_t n, uint2 *__restrict__ out) {
    static_assert(BYTES % 8 == 0 && BYTES <= NW * 64, "record size");
    u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u32 k = 0; k < 64; k++) {
        u32 gl = wave * 64 + k;
        int64_t gidx = base + gl;
        if (gidx >= n) break;
        for (u32 ch = lane; ch < BYTES / 8; ch += 64) {
            u32 b = (u32)(words[gl][ch >> 3] >> ((ch & 7) * 8)) & 255u;
            out[gidx * (BYTES / 8) + ch] = make_uint2(nibble_bytes(b), nibble_bytes(b >> 4));
        }
    }
}

// menjaj_talon_v_vektor (Igralec.py:535-543), the input of the exchange decision, for the games that
// wait for tarok_exchange: [roka 54 | talon (54,6) flattened card-major | igra one-hot 15 | pad 7]
// = 400 bytes of 0/1; zeros for games in any other phase.
TK_KERNEL(TK_BLOCK, 64) void k_observe_exchange_ref(int64_t n, const ulonglong2 *__restrict__ s01,
                                                                  const ulonglong2 *__restrict__ s23, uint2 *__restrict__ out) {
    TK_VGPR_TOP(64, 63);
    __shared__ u64 words[TK_BLOCK][7];
    int64_t base = (int64_t)blockIdx.x * TK_BLOCK, i = base + threadIdx.x;
    Game g;
    load_game(g, s01, s23, i < n ? i : n - 1);
    u64 w[7] = {0, 0, 0, 0, 0, 0, 0};
    if (i < n && g.phase == TK_PHASE_EXCHANGE) {
        u32 gs = group_size(g.contract);
        bits_insert<0>(w, hand_of(g, g.declarer));                        // :540 (the hand before the exchange)
#pragma unroll
        for (u32 r = 0; r < 6; r++) bits_set(w, 54 + (u32)((g.talon >> (6 * r)) & 63) * 6 + r / gs);   // :541-542
        // igra_zalozi2index (Igralec.py:717-745): Tri/Dve/Ena x suit -> 0..11, Solo_tri/dve/ena -> 12..14
        u32 idx = has_king(g.contract) ? (g.contract - 1) * 4 + g.king : 12 + (g.contract - TK_SOLO_TRI);
        bits_set(w, 378 + idx);                                           // :539
    }
#pragma unroll
    for (int k = 0; k < 7; k++) words[threadIdx.x][k] = w[k];
    __syncthreads();
    write_bit_records<7, TAROK_REF_EXCHANGE_BYTES>(words, base, n, out);
}

// The bidding input (pripavi_licitiram, Igralec.py:278-281): every seat's hand as 54 bytes of 0/1,
// [N][4][54].
TK_KERNEL(TK_BLOCK, 64) void k_observe_hands_ref(int64_t n, const ulonglong2 *__restrict__ s01,
                                                               const ulonglong2 *__restrict__ s23, uint2 *__restrict__ out) {
    TK_VGPR_TOP(64, 63);
    __shared__ u64 words[TK_BLOCK][4];
    int64_t base = (int64_t)blockIdx.x * TK_BLOCK, i = base + threadIdx.x;
    Game g;
    load_game(g, s01, s23, i < n ? i : n - 1);
    u64 w[4] = {0, 0, 0, 0};
    if (i < n) {
        bits_insert<0>(w, hand_of(g, 0)); bits_insert<54>(w, hand_of(g, 1));
        bits_insert<108>(w, hand_of(g, 2)); bits_insert<162>(w, hand_of(g, 3));
    }
#pragma unroll
    for (int k = 0; k < 4; k++) words[threadIdx.x][k] = w[k];
    __syncthreads();
    write_bit_records<4, 216>(words, base, n, out);
}

// Masked categorical sample from policy logits, one thread per game: softmax over the legal
// cards only (mask = observation word), inverse-CDF draw with the spec RNG (draw 192 + cards
// played), log-probability of the drawn card.  Replaces ~10 framework kernels per step
// (bit-expand mask, masked_fill, log_softmax, multinomial, gather) with one pass over 8 MB.
__device__ __forceinline__ float bf16_to_f32(u32 h) { return __uint_as_float(h << 16); }

// The play mode of the MODE = 1 kernels (tarok_set_play_mode; include/tarok_env.h): the tempered softmax
// exp((l - max) * inv_t), or with `greedy` the lowest-numbered legal card at the maximum; with thr > 0 a coin — spec
// RNG draw 256 + cards played, explore iff (coin >> 8) < thr — sends the game to the Bot's card (policy_action, draw
// 128 + cards played); eps = thr / 2^24, the probability of that.  The log-probability is that of the card played under
// the whole mode: log((1 - eps) p_T(card) + eps / k), k legal cards.  MODE = 0 is the plain draw at (1, 0) and takes none
// of this: everything a mode adds sits behind `if constexpr (MODE)`.
struct PlayMode { float inv_t; int greedy; u32 thr; float eps; };
#define TK_DRAW_EXPLORE 256u

template <int MODE>
__device__ __forceinline__ void sample_body(int64_t n, const uint4 *logits /* [N,64] bf16 */, const u64 *obs, const u64 *gkey,
                                            uint8_t *action, float *logp, const PlayMode pm = PlayMode{}) {
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 o = obs[i];
    u64 m = o & TAROK_OBS_MASK;
    if (!m) { action[i] = 255; if (logp) logp[i] = 0.f; return; }
    float l[56];
#pragma unroll
    for (int q = 0; q < 7; q++) {
        uint4 v = logits[i * 8 + q];
        u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            l[q * 8 + 2 * k] = bf16_to_f32(w[k] & 0xFFFFu);
            l[q * 8 + 2 * k + 1] = bf16_to_f32(w[k] >> 16);
        }
    }
    float mx = -3.0e38f;
#pragma unroll
    for (int c = 0; c < 54; c++) mx = ((m >> c) & 1) ? fmaxf(mx, l[c]) : mx;
    int best = -1;                     // MODE: the lowest-numbered legal card at the maximum (strictly greater moves it)
    if constexpr (MODE) {
        float bm = -3.0e38f;
#pragma unroll
        for (int c = 0; c < 54; c++) {
            bool up = ((m >> c) & 1) && (best < 0 || l[c] > bm);
            bm = up ? l[c] : bm;
            best = up ? c : best;
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < 54; c++) {
        float e;
        if constexpr (MODE) e = ((m >> c) & 1) ? __expf((l[c] - mx) * pm.inv_t) : 0.f;
        else e = ((m >> c) & 1) ? __expf(l[c] - mx) : 0.f;
        l[c] = e;                      // keep exp() for the draw
        sum += e;
    }
    u32 r = rng32(gkey[i], 192u + ((u32)(o >> TAROK_OBS_STEP_SHIFT) & 63u));
    float u = ((float)(r >> 8) + 0.5f) * (1.0f / 16777216.0f) * sum;
    float acc = 0.f, pe = 0.f;
    int pickc = -1;
#pragma unroll
    for (int c = 0; c < 54; c++) {
        bool legal = (m >> c) & 1;
        acc += l[c];
        bool take = legal && pickc < 0 && acc > u;
        pe = take ? l[c] : pe;
        pickc = take ? c : pickc;
    }
    if (pickc < 0) {                   // rounding at the top end: the last legal card
        pickc = 63 - __clzll(m);
        pe = l[53];
#pragma unroll
        for (int c = 0; c < 54; c++) pe = (c == pickc) ? l[c] : pe;
    }
    if constexpr (MODE) {
        const u32 played = (u32)(o >> TAROK_OBS_STEP_SHIFT) & 63u;
        const int bc = (int)policy_action(gkey[i], played, m);      // the Bot's card here
        float pb = 0.f;
#pragma unroll
        for (int c = 0; c < 54; c++) pb = (c == bc) ? l[c] : pb;
        if (pm.greedy) { pickc = best; pe = 1.f; sum = 1.f; pb = bc == best ? 1.f : 0.f; }
        if (pm.thr && (rng32(gkey[i], TK_DRAW_EXPLORE + played) >> 8) < pm.thr) { pickc = bc; pe = pb; }
        action[i] = (uint8_t)pickc;
        if (logp) logp[i] = __logf((1.f - pm.eps) * (pe / sum) + pm.eps / (float)popc64(m));
        return;
    }
    action[i] = (uint8_t)pickc;
    if (logp) logp[i] = __logf(pe / sum);
}

TK_KERNEL(TK_BLOCK, 256) void k_sample(int64_t n, const uint4 *__restrict__ logits /* [N,64] bf16 */,
                                                    const u64 *__restrict__ obs, const u64 *__restrict__ gkey,
                                                    uint8_t *__restrict__ action, float *__restrict__ logp) {
    TK_VGPR_TOP(256, 255);
    sample_body<0>(n, logits, obs, gkey, action, logp);
}

TK_KERNEL(TK_BLOCK, 256) void k_sample_mode(int64_t n, const uint4 *__restrict__ logits /* [N,64] bf16 */,
                                                         const u64 *__restrict__ obs, const u64 *__restrict__ gkey,
                                                         uint8_t *__restrict__ action, float *__restrict__ logp,
                                                         float inv_t, int greedy, u32 thr, float eps) {
    TK_VGPR_TOP(256, 255);
    sample_body<1>(n, logits, obs, gkey, action, logp, PlayMode{inv_t, greedy, thr, eps});
}


// ---------------------------------------------------------------------------
// Learner side: a minibatch of network inputs from the rollout's 32-byte feature words
// (tarok_policy_mlp / tarok_policy_step feature_words_out): out[j] = the 256 bf16 0/1 features
// of sample index[j] (or of sample j when index is NULL).  One 16-byte chunk (one byte of a
// feature word -> 8 bf16) per thread, 32 threads per sample: the gather and the expansion in one
// pass, full 512-byte rows written per 32 lanes.
TK_KERNEL(TK_BLOCK, 64) void k_expand_features(int64_t n, const u64 *__restrict__ words /* [.,4] */,
                                                             const int64_t *__restrict__ index, uint4 *__restrict__ out) {
    TK_VGPR_TOP(64, 63);
    int64_t t = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    int64_t j = t >> 5;
    if (j >= n) return;
    u32 chunk = (u32)t & 31;
    int64_t src = index ? index[j] : j;
    u32 byte = reinterpret_cast<const uint8_t *>(words + src * 4)[chunk];
    uint4 v;
    v.x = ((byte & 1) ? 0x3F80u : 0u) | ((byte & 2) ? 0x3F800000u : 0u);
    v.y = ((byte & 4) ? 0x3F80u : 0u) | ((byte & 8) ? 0x3F800000u : 0u);
    v.z = ((byte & 16) ? 0x3F80u : 0u) | ((byte & 32) ? 0x3F800000u : 0u);
    v.w = ((byte & 64) ? 0x3F80u : 0u) | ((byte & 128) ? 0x3F800000u : 0u);
    out[j * 32 + chunk] = v;
}

// Block sum of three per-thread terms: part[blockIdx.x] = {sum s0, sum s1, sum s2, 0} over the workgroup, in a fixed
// order (wave butterfly 32 .. 1, then the four waves in index order by thread 0): the result does not depend on the
// schedule.  Every thread of the workgroup calls it.  Used by k_ppo_loss and the returns kernels (tarok_learner.inc).
__device__ __forceinline__ void block_sum3(float s0, float s1, float s2, float4 *__restrict__ part) {
    __shared__ float red[3][TK_BLOCK / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s0; red[1][threadIdx.x >> 6] = s1; red[2][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int k = 0; k < TK_BLOCK / 64; k++) { a0 += red[0][k]; a1 += red[1][k]; a2 += red[2][k]; }
        part[blockIdx.x] = make_float4(a0, a1, a2, 0.f);
    }
}

// ---------------------------------------------------------------------------
// Learner side of the policy step: the clipped-surrogate policy-gradient loss
// over the LEGAL cards, forward and gradient in one pass over the head outputs.  Replaces ~40
// framework elementwise kernels per minibatch (bit-expand of the mask, masked_fill, log_softmax,
// gather, exp, clamp, min, entropy, their backward kernels) with one read of [B,64] bf16 and one
// write of the same shape.
//   out [B,64] bf16: columns 0..53 card logits, column 54 the state value.
//   per sample: pi = -min(r A, clamp(r, 1-eps, 1+eps) A) with r = exp(logp[a] - logp_old),
//               v = (value - ret)^2,  H = -sum p log p over the legal cards;
//   loss = sum_i w_i (pi_i + vf v_i - ent H_i) / wsum.
// dout = d loss / d out (bf16); part[block] = {sum w pi, sum w v, sum w H, 0} (f32, unscaled).
TK_KERNEL(TK_BLOCK, 256) void k_ppo_loss(int64_t n, const uint4 *__restrict__ out, const u64 *__restrict__ words,
                                                      const int64_t *__restrict__ act, const float *__restrict__ logp_old,
                                                      const float *__restrict__ adv, const float *__restrict__ ret,
                                                      const float *__restrict__ weight, float clip, float vf_coef,
                                                      float ent_coef, const float *__restrict__ inv_wsum_p, uint4 *__restrict__ dout,
                                                      float4 *__restrict__ part) {
    TK_VGPR_TOP(256, 255);
    float inv_wsum = *inv_wsum_p;
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    float s_pi = 0.f, s_v = 0.f, s_h = 0.f;
    if (i < n) {
        float l[64];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            uint4 v = out[i * 8 + q];
            u32 wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                l[q * 8 + 2 * k] = bf16_to_f32(wv[k] & 0xFFFFu);
                l[q * 8 + 2 * k + 1] = bf16_to_f32(wv[k] >> 16);
            }
        }
        u64 m = words[i] & TAROK_OBS_MASK;
        float w = weight[i];
        if (!m) { m = 1; w = 0.f; }                        // nothing to play: no contribution, finite arithmetic
        float ws = w * inv_wsum;
        u32 a = (u32)act[i];
        a = a < 54 ? a : 53u;                              // (rows without a card carry weight 0)
        float value = l[54];
        float mx = -3.0e38f;
#pragma unroll
        for (int c = 0; c < 54; c++) mx = ((m >> c) & 1) ? fmaxf(mx, l[c]) : mx;
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 54; c++) {
            float e = ((m >> c) & 1) ? __expf(l[c] - mx) : 0.f;
            l[c] = e;
            sum += e;
        }
        float ls = __logf(sum), inv = 1.0f / sum;
        // probabilities in place; entropy; log-prob of the played card
        float H = 0.f, la = 0.f;
#pragma unroll
        for (int c = 0; c < 54; c++) {
            float p = l[c] * inv;
            float lp = p > 0.f ? __logf(l[c]) - ls : 0.f;  // log p_c (0 where p_c = 0: p log p -> 0)
            H -= p * lp;
            la = (c == (int)a) ? __logf(fmaxf(l[c], 1e-38f)) - ls : la;
            l[c] = p;
        }
        float r = __expf(la - logp_old[i]);
        float A = adv[i];
        float rc = fminf(fmaxf(r, 1.0f - clip), 1.0f + clip);
        float s1 = r * A, s2 = rc * A;
        bool first = s1 <= s2;                              // which branch of the min is active
        bool inside = r > 1.0f - clip && r < 1.0f + clip;
        float g = (first || inside) ? -A * r : 0.f;         // d pi / d logp[a]
        float dv = value - ret[i];
        s_pi = w * (-fminf(s1, s2));
        s_v = w * dv * dv;
        s_h = w * H;
        // d loss / d logit_c = ws [ g (delta_ca - p_c) + ent p_c (log p_c + H) ] on the legal cards
#pragma unroll
        for (int c = 0; c < 54; c++) {
            float p = l[c];
            float lp = p > 0.f ? __logf(p) : 0.f;
            float d = g * (((c == (int)a) ? 1.0f : 0.0f) - p) + ent_coef * p * (lp + H);
            l[c] = ((m >> c) & 1) ? ws * d : 0.f;
        }
        l[54] = ws * vf_coef * 2.0f * dv;
#pragma unroll
        for (int c = 55; c < 64; c++) l[c] = 0.f;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            uint4 v;
            u32 wv[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                __bf16 lo = (__bf16)l[q * 8 + 2 * k], hi = (__bf16)l[q * 8 + 2 * k + 1];
                wv[k] = (u32)__builtin_bit_cast(unsigned short, lo) | ((u32)__builtin_bit_cast(unsigned short, hi) << 16);
            }
            v.x = wv[0]; v.y = wv[1]; v.z = wv[2]; v.w = wv[3];
            dout[i * 8 + q] = v;
        }
    }
    block_sum3(s_pi, s_v, s_h, part);
}

// ---------------------------------------------------------------------------
// Fused policy step for a learner: observation features -> MLP 256-256-256-64
// (bf16 MFMA, f32 accumulate) -> masked categorical sample, in ONE launch.  The features never
// leave the chip (built in LDS from the 32-byte packed state), the activations go LDS -> MFMA ->
// LDS, only action / log-prob / value (+ optionally the features, for the learner's update) are
// written.  Replaces tarok_observe + 4 framework GEMMs + bias/ReLU kernels + tarok_sample_policy
// (~150 MB of activation traffic per 65,536 games) — the one place in this build where work is
// GEMM shaped, so the one place that uses the matrix cores.
//
// Workgroup = 256 threads = 4 waves, 128 games, ONE activation buffer X[game][feature] in LDS
// (row stride 264 bf16 = 528 B) updated in place, 72 KB per workgroup: two workgroups share a CU
// (two waves per SIMD), so one's feature build / epilogues / sampling run under the other's MFMAs.
// Every layer is computed TRANSPOSED, D[feature][game] = W[feature][k] * X^T[k][game], with
// v_mfma_f32_32x32x16_bf16: lane l (r = l & 31, h = l >> 5) supplies A[row r][k = 8h..8h+7] = one
// 16-byte piece of the weight (pre-arranged in fragment order: a wave's load is 1 KiB contiguous)
// and B[k = 8h..8h+7][col r] = 16 contiguous bytes of game r's row in LDS; it receives
// D[(reg & 3) + 8 (reg >> 2) + 4 h][col r]: four CONSECUTIVE features of one game per register
// quad, i.e. one 8-byte LDS store of packed bf16 per quad (the untransposed product scatters 2-byte
// stores).  Layers 1-2: wave w owns features [64w, 64w+64) x all 128 games (2 x 4 tiles, 128 MFMAs,
// the weight slab streamed from L2 four k-steps ahead); layer 3 (64 outputs = 54 card logits, value
// in column 54): wave w owns games [32w, 32w+32).
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
#define PM_M 128
// the eight bits of a byte as eight bf16 0.0 / 1.0 (16 bytes): bit k of b lands on bit 8k of (b * 0x204081) (copies of b at shifts
// 0, 7, 14, 21), a byte permute puts two of those bytes into the halves of a word, times 0x3F80 — 13 instructions per byte where
// a select per bit takes 28 (the learner's kernels expand their feature words with it too)
__device__ __forceinline__ uint4 tk_expand_byte(u32 b) {
    u32 lo = __umul24(b & 15u, 0x204081u) & 0x01010101u;        // byte k = bit k
    u32 hi = __umul24(b >> 4, 0x204081u) & 0x01010101u;         // byte k = bit 4 + k
    uint4 v;
    v.x = __umul24(__builtin_amdgcn_perm(0u, lo, 0x0C010C00u), 0x3F80u);   // bytes {lo.0, 0, lo.1, 0}
    v.y = __umul24(__builtin_amdgcn_perm(0u, lo, 0x0C030C02u), 0x3F80u);
    v.z = __umul24(__builtin_amdgcn_perm(0u, hi, 0x0C010C00u), 0x3F80u);
    v.w = __umul24(__builtin_amdgcn_perm(0u, hi, 0x0C030C02u), 0x3F80u);
    return v;
}
#define PM_LD 264
#define PM_LL 68             // f32 logits row stride (272 B: float4 stores stay aligned)

// the weight fragments of a wave's first four k-steps (issued early by the caller: before the
// feature build for layer 1, before the previous layer's epilogue for layer 2)
__device__ __forceinline__ void mlp_prefetch(bf16x8 (&wq)[4][2], const __bf16 *__restrict__ w, u32 first_tile) {
    const bf16x8 *wf = reinterpret_cast<const bf16x8 *>(w) + (size_t)first_tile * 16 * 64 + __lane_id();
#pragma unroll
    for (int d = 0; d < 4; d++)
#pragma unroll
        for (int ft = 0; ft < 2; ft++) wq[d][ft] = wf[(ft * 16 + d) * 64];
    __builtin_amdgcn_sched_barrier(0);
}

// (X: the 128-game tile of this wave; wave = 0..3 within the tile; the barriers are workgroup-wide)
__device__ __forceinline__ void mlp_hidden(__bf16 *__restrict__ X, const __bf16 *__restrict__ w, const float *__restrict__ bias,
                                           bf16x8 (&wq)[4][2], u32 wave) {
    u32 lane = __lane_id(), r = lane & 31, h = lane >> 5;
    const bf16x8 *wf = reinterpret_cast<const bf16x8 *>(w) + (size_t)(wave * 2) * 16 * 64 + lane;
    f32x16 acc[2][4];
#pragma unroll
    for (int ft = 0; ft < 2; ft++)
#pragma unroll
        for (int gt = 0; gt < 4; gt++)
#pragma unroll
            for (int j = 0; j < 16; j++) acc[ft][gt][j] = 0.f;
    bf16x8 xn[4];                                      // activations one k-step ahead (wq: weights, 4 k-steps in flight)
#pragma unroll
    for (int gt = 0; gt < 4; gt++) xn[gt] = *reinterpret_cast<const bf16x8 *>(X + (32 * gt + r) * PM_LD + 8 * h);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < 16; kk++) {
        bf16x8 x[4] = {xn[0], xn[1], xn[2], xn[3]};
        bf16x8 wc[2] = {wq[kk & 3][0], wq[kk & 3][1]};
        if (kk + 4 < 16) {
#pragma unroll
            for (int ft = 0; ft < 2; ft++) wq[kk & 3][ft] = wf[(ft * 16 + kk + 4) * 64];
        }
        if (kk < 15) {
#pragma unroll
            for (int gt = 0; gt < 4; gt++) xn[gt] = *reinterpret_cast<const bf16x8 *>(X + (32 * gt + r) * PM_LD + 16 * (kk + 1) + 8 * h);
        }
#pragma unroll
        for (int ft = 0; ft < 2; ft++)
#pragma unroll
            for (int gt = 0; gt < 4; gt++) acc[ft][gt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc[ft], x[gt], acc[ft][gt], 0, 0, 0);
        // keep the loads issued in this k-step here: left alone, the scheduler sinks each weight
        // load to just before its use (to save registers) and every k-step waits out an L2 round trip
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                                   // every wave has read its last X fragment
#pragma unroll
    for (int ft = 0; ft < 2; ft++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            u32 f0 = wave * 64 + 32 * ft + 8 * q + 4 * h;
            float4 bv = *reinterpret_cast<const float4 *>(bias + f0);
#pragma unroll
            for (int gt = 0; gt < 4; gt++) {
                bf16x4 o;
                o[0] = (__bf16)fmaxf(acc[ft][gt][4 * q + 0] + bv.x, 0.f);
                o[1] = (__bf16)fmaxf(acc[ft][gt][4 * q + 1] + bv.y, 0.f);
                o[2] = (__bf16)fmaxf(acc[ft][gt][4 * q + 2] + bv.z, 0.f);
                o[3] = (__bf16)fmaxf(acc[ft][gt][4 * q + 3] + bv.w, 0.f);
                *reinterpret_cast<bf16x4 *>(X + (32 * gt + r) * PM_LD + f0) = o;
            }
        }
    __syncthreads();
}

// The weights of one network, as tarok_policy_mlp takes them (bf16 in MFMA fragment order, f32 biases).
struct PolicyWeights {
    const __bf16 *w1; const float *b1; const __bf16 *w2; const float *b2; const __bf16 *w3; const float *b3;
};

// The feature words ext[game][4] expanded to bf16 0.0 / 1.0 into X, one 16-byte chunk (8 features = one byte of a
// feature word) at a time.  Two threads per game (tid < 2 * games), thread parity p takes the odd / even bytes of the
// game's 32: ONE 32-byte LDS read per thread up front instead of a dependent byte read per chunk, and the pair's
// 16-byte stores fall into different banks.  (A 256-entry LDS table byte -> 8 bf16 was tried: no faster than the selects.)
// (k_learn_chain restates it: through this function that tuned kernel compiles to another instruction stream.)
__device__ __forceinline__ void policy_expand(__bf16 *X, const u64 (*ext)[4], u32 tid) {
    u32 gme = tid >> 1, par = tid & 1;
    const uint4 *row = reinterpret_cast<const uint4 *>(&ext[gme][0]);
    uint4 r0 = row[0], r1 = row[1];
    u32 wd[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        u32 chunk = 2 * j + par;                       // byte `chunk` of the row = byte (2j + par) & 3 of word j / 2
        u32 byte = (wd[j >> 1] >> (8 * ((2 * (j & 1)) + par))) & 255u;
        *reinterpret_cast<uint4 *>(X + gme * PM_LD + 8 * chunk) = tk_expand_byte(byte);
    }
}

// Layer 3: 64 outputs; wave w of the tile takes games [32w, 32w+32), both 32-feature tiles; f32 logits to LDS
// [games][PM_LL] OVER the activation buffer (Xt: this tile's rows of it, L: all of it as floats — the same memory,
// hence the barrier between the last read and the first store, and no __restrict__ on either).
__device__ __forceinline__ void mlp_head(const __bf16 *Xt, float *L, const __bf16 *__restrict__ w3, const float *__restrict__ b3,
                                         u32 wave, u32 tile) {
    u32 lane = __lane_id(), r = lane & 31, h = lane >> 5;
    const bf16x8 *wf = reinterpret_cast<const bf16x8 *>(w3) + lane;
    f32x16 acc[2];
#pragma unroll
    for (int ft = 0; ft < 2; ft++)
#pragma unroll
        for (int j = 0; j < 16; j++) acc[ft][j] = 0.f;
    bf16x8 wq[4][2];
#pragma unroll
    for (int d = 0; d < 4; d++)
#pragma unroll
        for (int ft = 0; ft < 2; ft++) wq[d][ft] = wf[(ft * 16 + d) * 64];
    bf16x8 xn = *reinterpret_cast<const bf16x8 *>(Xt + (32 * wave + r) * PM_LD + 8 * h);
#pragma unroll
    for (int kk = 0; kk < 16; kk++) {
        bf16x8 x = xn;
        bf16x8 wc[2] = {wq[kk & 3][0], wq[kk & 3][1]};
        if (kk + 4 < 16) {
#pragma unroll
            for (int ft = 0; ft < 2; ft++) wq[kk & 3][ft] = wf[(ft * 16 + kk + 4) * 64];
        }
        if (kk < 15) xn = *reinterpret_cast<const bf16x8 *>(Xt + (32 * wave + r) * PM_LD + 16 * (kk + 1) + 8 * h);
#pragma unroll
        for (int ft = 0; ft < 2; ft++) acc[ft] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc[ft], x, acc[ft], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                                   // all waves are done with X: the logits may overwrite it
#pragma unroll
    for (int ft = 0; ft < 2; ft++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            u32 f0 = 32 * ft + 8 * q + 4 * h;
            float4 bv = *reinterpret_cast<const float4 *>(b3 + f0);
            float4 o = make_float4(acc[ft][4 * q + 0] + bv.x, acc[ft][4 * q + 1] + bv.y, acc[ft][4 * q + 2] + bv.z, acc[ft][4 * q + 3] + bv.w);
            *reinterpret_cast<float4 *>(L + (PM_M * tile + 32 * wave + r) * PM_LL + f0) = o;
        }
}

// The masked categorical sampler of the fused kernels (same draw, same order of additions as k_sample), two lanes per
// game: lane pair (2g, 2g+1) takes cards 0..26 / 27..53 (half = 0 / 1), partner values through DPP.  In two parts, so
// that a kernel with two networks reads a game's inputs once and samples once per network.

// the pair partner's value (quad_perm [1,0,3,2]; DPP reads need the source lane active: never inside a select)
__device__ __forceinline__ float pm_swap(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true)); }
__device__ __forceinline__ int pm_swap(int x) { return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true); }

struct PolicySampleIn {
    u64 o, m, key;            // the game's observation word, its legal cards, its draw key
    u32 played, mh;           // cards played so far in this game; the legality bits of this lane's cards
    int last;                 // the last legal card
};
struct PolicyPick {
    int pk; float pp, sum, v54;      // card, its exp(logit - max), the sum of those, the state value
    int bc; float pb;                // MODE only: the Bot's card on this position and its exp (PlayMode: an exploring game plays it)
};

__device__ __forceinline__ PolicySampleIn policy_sample_inputs(const u64 *__restrict__ obs, const u64 *__restrict__ gkey, int64_t i, u32 half) {
    PolicySampleIn in;
    in.o = obs[i];
    in.m = in.o & TAROK_OBS_MASK;
    in.key = gkey[i];
    in.played = (u32)(in.o >> TAROK_OBS_STEP_SHIFT) & 63u;
    in.mh = (u32)(in.m >> (27 * half)) & 0x7FFFFFFu;
    in.last = in.m ? 63 - __clzll(in.m) : 0;
    return in;
}

// one draw from logits row gi of L: the candidate is whole on the game's half == 0 lane
template <int MODE = 0>
__device__ __forceinline__ PolicyPick policy_sample(const float *L, u32 gi, u32 half, const PolicySampleIn &in, const PlayMode &pm = PlayMode{}) {
    float l[27];
#pragma unroll
    for (int c = 0; c < 27; c++) l[c] = L[gi * PM_LL + 27 * half + c];
    float v54 = L[gi * PM_LL + 54];
    const u32 mh = in.mh;
    float mx = -3.0e38f;
#pragma unroll
    for (int c = 0; c < 27; c++) mx = ((mh >> c) & 1) ? fmaxf(mx, l[c]) : mx;
    mx = fmaxf(mx, pm_swap(mx));
    // MODE: this lane's arg-max over its 27 cards (strictly greater moves it: the lowest index stays), before the logits
    // turn into exps
    int am = -1;
    float bm = -3.0e38f;
    if constexpr (MODE) {
#pragma unroll
        for (int c = 0; c < 27; c++) {
            bool up = ((mh >> c) & 1) && (am < 0 || l[c] > bm);
            bm = up ? l[c] : bm;
            am = up ? c : am;
        }
    }
#pragma unroll
    for (int c = 0; c < 27; c++) {
        if constexpr (MODE) l[c] = ((mh >> c) & 1) ? __expf((l[c] - mx) * pm.inv_t) : 0.f;
        else l[c] = ((mh >> c) & 1) ? __expf(l[c] - mx) : 0.f;
    }
    // running sums in card order: the low half from 0, then the high half from the low half's total
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 27; c++) s += l[c];
    float s_sw = pm_swap(s);
    float s_low = half ? s_sw : s;                         // sum over cards 0..26 (in both lanes)
    float start = half ? s_low : 0.f;
    float sum = start;
#pragma unroll
    for (int c = 0; c < 27; c++) sum += l[c];
    float sum_sw = pm_swap(sum);
    sum = half ? sum : sum_sw;                             // total over cards 0..53, from the high lane
    u32 rr = rng32(in.key, 192u + in.played);
    float u = ((float)(rr >> 8) + 0.5f) * (1.0f / 16777216.0f) * sum;
    float acc = start, pe = 0.f;
    int pickc = -1;
#pragma unroll
    for (int c = 0; c < 27; c++) {
        bool legal = (mh >> c) & 1;
        acc += l[c];
        bool take = legal && pickc < 0 && acc > u;
        pe = take ? l[c] : pe;
        pickc = take ? c : pickc;
    }
    // rounding at the top end: the last legal card (its lane supplies the probability)
    const int last = in.last;
    float pl = 0.f;
#pragma unroll
    for (int c = 0; c < 27; c++) pl = (c + 27 * (int)half == last) ? l[c] : pl;
    int pick_o = pm_swap(pickc);
    float pe_o = pm_swap(pe), pl_o = pm_swap(pl);
    PolicyPick p;
    p.pk = pickc >= 0 ? pickc : (pick_o >= 0 ? pick_o + 27 : last);
    p.pp = pickc >= 0 ? pe : (pick_o >= 0 ? pe_o : (last < 27 ? pl : pl_o));
    p.sum = sum;
    p.v54 = v54;
    if constexpr (MODE) {
        // the Bot's card of the position (the same in both lanes: whole on the half == 0 lane) and its exp from the lane
        // that holds it; the pair's arg-max, the low half winning ties.  Every partner read is made before any select.
        const int bc = (int)policy_action(in.key, in.played, in.m);
        float pb = 0.f;
#pragma unroll
        for (int c = 0; c < 27; c++) pb = (c + 27 * (int)half == bc) ? l[c] : pb;
        const float pb_o = pm_swap(pb), bm_o = pm_swap(bm);
        const int am_o = pm_swap(am);
        const int best = (am >= 0 && (am_o < 0 || bm >= bm_o)) ? am : am_o + 27;
        p.bc = bc;
        p.pb = bc < 27 ? pb : pb_o;
        if (pm.greedy) { p.pk = best; p.pp = 1.f; p.sum = 1.f; p.pb = bc == best ? 1.f : 0.f; }
    }
    return p;
}

// The policy step of 128 * TILES games by a workgroup of 256 * TILES threads (tile t = waves 4t..4t+3 and rows 128t..
// of X): the ONE forward and sampler of tarok_policy_mlp (TILES = 1) and of the three tarok_policy_step launches
// (TILES = 2, which then need the sampled cards of their 256 games in LDS: act_s).  The feature words are built once
// into ext; then, ONCE PER NETWORK, the activation buffer is expanded from ext and run through layers 1-3 and the
// sampler (the logits of a pass overwrite the activations, and no second buffer fits in LDS); one block writes out.
// NETS = 2 (tarok_policy_step_versus): nets[0] plays the seats of a game's seat set (seat_sets[i], or `seats` for every
// game), nets[1] the others; both are evaluated for every game (the seat to move differs from lane to lane: nothing
// wave-uniform to skip), the mover's network's candidate waits in the registers of the game's half == 0 lane.  Every
// pass is the same code in the same order of accumulation, so a network's card, log-probability and value are the bits
// of tarok_policy_mlp with its weights.  With NETS = 1 the loop and the selects fold away.
// MIXED (tarok_policy_step_seats): a game whose seat to move is not in its seat set takes the Bot's card — k_policy's,
// i.e. what tarok_step_random plays — and the log-probability 0; the network is evaluated for every game all the same.
// MODE = 1 (the *_mode kernels): the env's play mode, PlayMode — tempered or greedy card, the exploration coin and the
// mode's log-probability at the write-out, on the half == 0 lane; a Bot seat of a mixed table is the Bot's all the same.
template <int TILES, int NETS = 1, bool MIXED = false, int MODE = 0>
__device__ __forceinline__ void policy_body(
    int64_t n, const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23, const u64 *__restrict__ obs,
    const u64 *__restrict__ gkey, const PolicyWeights (&nets)[NETS], uint8_t *__restrict__ action, float *__restrict__ logp,
    float *__restrict__ value, uint4 *__restrict__ features_out, ulonglong2 *__restrict__ feature_words_out,
    u64 *__restrict__ stamps, uint8_t *__restrict__ act_s,
    u32 **lds_after = nullptr /* the activation buffer: free once every thread has returned */, u32 seats = 15,
    const uint8_t *__restrict__ seat_sets = nullptr, const PlayMode pmode = PlayMode{}) {
    constexpr int GAMES = PM_M * TILES;
    u64 ts[7];
#define PM_STAMP(k) if (stamps) ts[k] = __builtin_amdgcn_s_memtime();
    PM_STAMP(0)
    __shared__ __attribute__((aligned(16))) __bf16 X[GAMES * PM_LD];
    __shared__ u64 ext[GAMES][4];
    int64_t base = (int64_t)blockIdx.x * GAMES;
    u32 tid = threadIdx.x, wave4 = (tid >> 6) & 3, tile = tid >> 8;
    __bf16 *Xt = X + tile * PM_M * PM_LD;
    float *L = reinterpret_cast<float *>(X);
    if (lds_after) *lds_after = reinterpret_cast<u32 *>(X);
    bf16x8 wq[4][2];
    mlp_prefetch(wq, nets[0].w1, wave4 * 2);   // lands while the features are built
    if (tid < GAMES) {
        int64_t i = base + tid < n ? base + tid : n - 1;
        Game g;
        load_game(g, s01, s23, i);
        policy_feature_words(g, ext[tid]);
        if (feature_words_out && base + tid < n) {
            feature_words_out[i * 2] = make_ulonglong2(ext[tid][0], ext[tid][1]);
            feature_words_out[i * 2 + 1] = make_ulonglong2(ext[tid][2], ext[tid][3]);
        }
    }
    // the sampler's game (two lanes per game) and whether its seat to move is in its seat set
    const u32 gi = tid >> 1, half = tid & 1;
    const bool in_range = base + gi < n;
    const int64_t i = in_range ? base + gi : n - 1;
    auto in_set = [&](u64 o) {
        u32 set = seat_sets ? seat_sets[i] : seats;
        return ((set >> ((u32)(o >> TAROK_OBS_SEAT_SHIFT) & 3u)) & 1u) != 0;
    };
    PolicySampleIn in;
    bool is_a = true;
    if constexpr (NETS > 1) {                      // (the same for both passes)
        in = policy_sample_inputs(obs, gkey, i, half);
        is_a = in_set(in.o);
    }
    PolicyPick pick = {0, 0.f, 1.f, 0.f, 0, 0.f};  // the mover's network's candidate
    auto pass = [&](int net) __attribute__((always_inline)) {
        PolicyWeights w = nets[0];
        if constexpr (NETS > 1) { if (net) w = nets[1]; }
        // (the feature words are in ext; pass 1: every lane has read its logits of pass 0 before the activations go
        // back over them)
        __syncthreads();
        PM_STAMP(6)
        if (net) mlp_prefetch(wq, w.w1, wave4 * 2);
        policy_expand(X, ext, tid);
        if (features_out) {                                    // optional global copy: full 512-byte rows per 32 lanes
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 16; it++) {
                u32 gme = it * (8 * TILES) + (tid >> 5), chunk = tid & 31;
                if (base + gme < n) features_out[(base + gme) * 32 + chunk] = *reinterpret_cast<const uint4 *>(X + gme * PM_LD + 8 * chunk);
            }
        }
        __syncthreads();
        PM_STAMP(1)
        mlp_hidden(Xt, w.w1, w.b1, wq, wave4);
        PM_STAMP(2)
        mlp_prefetch(wq, w.w2, wave4 * 2);
        mlp_hidden(Xt, w.w2, w.b2, wq, wave4);
        PM_STAMP(3)
        mlp_head(Xt, L, w.w3, w.b3, wave4, tile);
        __syncthreads();
        PM_STAMP(4)
        if (stamps && tid == 0) {
            for (int k = 0; k < 5; k++) stamps[blockIdx.x * 8 + k] = ts[k];
            stamps[blockIdx.x * 8 + 6] = ts[6];
        }
        if constexpr (NETS == 1) in = policy_sample_inputs(obs, gkey, i, half);
        PolicyPick c = policy_sample<MODE>(L, gi, half, in, pmode);
        const bool mine = NETS == 1 || (net == 0) == is_a;
        pick.pk = mine ? c.pk : pick.pk;
        pick.pp = mine ? c.pp : pick.pp;
        pick.sum = mine ? c.sum : pick.sum;
        pick.v54 = mine ? c.v54 : pick.v54;
        if constexpr (MODE) {
            pick.bc = c.bc;                        // (the position's, whichever network)
            pick.pb = mine ? c.pb : pick.pb;
        }
    };
    if constexpr (NETS == 1) pass(0);              // (no loop at all: nothing of the sampler is hoisted over the layers)
    else {
#pragma unroll 1
        for (int net = 0; net < NETS; net++) pass(net);
    }
    if (half == 0 && in_range) {
        const u64 m = in.m;
        if (value) value[i] = pick.v54;
        bool bot = false;
        if constexpr (MIXED) {
            bot = !in_set(in.o);
            if (bot && m) pick.pk = (int)policy_action(in.key, in.played, m);
        }
        if constexpr (MODE) {
            // the coin of an exploring mode (a network seat's only); the card's probability under the whole mode
            if (m && !bot && pmode.thr && (rng32(in.key, TK_DRAW_EXPLORE + in.played) >> 8) < pmode.thr) {
                pick.pk = pick.bc;
                pick.pp = pick.pb;
            }
            if (!m) { action[i] = 255; if (logp) logp[i] = 0.f; }
            else {
                action[i] = (uint8_t)pick.pk;
                if (logp) logp[i] = bot ? 0.f : __logf((1.f - pmode.eps) * (pick.pp / pick.sum) + pmode.eps / (float)popc64(m));
            }
        } else {
            if (!m) { action[i] = 255; if (logp) logp[i] = 0.f; }
            else {
                action[i] = (uint8_t)pick.pk;
                if (logp) logp[i] = bot ? 0.f : __logf(pick.pp / pick.sum);
            }
        }
        if (act_s) act_s[gi] = m ? (uint8_t)pick.pk : (uint8_t)255;
    }
    if (stamps && tid == 0) stamps[blockIdx.x * 8 + 5] = __builtin_amdgcn_s_memtime();
#undef PM_STAMP
}

__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_policy_mlp(
    int64_t n, const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23, const u64 *__restrict__ obs,
    const u64 *__restrict__ gkey, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3,
    const float *__restrict__ b3, uint8_t *__restrict__ action, float *__restrict__ logp, float *__restrict__ value,
    uint4 *__restrict__ features_out, ulonglong2 *__restrict__ feature_words_out, u64 *__restrict__ stamps) {
    TK_VGPR_TOP(256, 255);
    const PolicyWeights nets[1] = {{w1, b1, w2, b2, w3, b3}};
    policy_body<1>(n, s01, s23, obs, gkey, nets, action, logp, value, features_out, feature_words_out, stamps, nullptr);
}

__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_policy_mlp_mode(
    int64_t n, const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23, const u64 *__restrict__ obs,
    const u64 *__restrict__ gkey, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3,
    const float *__restrict__ b3, uint8_t *__restrict__ action, float *__restrict__ logp, float *__restrict__ value,
    uint4 *__restrict__ features_out, ulonglong2 *__restrict__ feature_words_out, u64 *__restrict__ stamps,
    float inv_t, int greedy, u32 thr, float eps) {
    TK_VGPR_TOP(256, 255);
    const PolicyWeights nets[1] = {{w1, b1, w2, b2, w3, b3}};
    policy_body<1, 1, false, 1>(n, s01, s23, obs, gkey, nets, action, logp, value, features_out, feature_words_out, stamps, nullptr,
                                nullptr, 15, nullptr, PlayMode{inv_t, greedy, thr, eps});
}

// tarok_bid_values: the bidding head — k_policy_mlp's forward (TILES = 1, the shared functions unchanged) on the twelve
// cards of a hand.  A workgroup takes 32 games = 128 rows, row = 4 * local game + seat: threads below 128 build ext[row] =
// bid_feature_words(the seat's hand, from k_bid_deal's buffer) under w1's prefetch; after the head, two lanes per row
// (lane parity p: pieces p, p + 2, p + 4 of the row's five) turn outputs 0..18 into the row's twenty values — scaled,
// clamped to +-2^30 (fmaxf first: a NaN becomes -2^30) and rounded to even — with tarok_playout_bids' zeros: a seat
// outside the game's set, a row outside `contracts`, row 19, an invalid deal (all four hands zero).  A ragged last
// workgroup's rows read game n - 1 and store nothing.  The env's games are not read.
__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_bid_values(
    int64_t n, const u64 *__restrict__ deal, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3,
    const float *__restrict__ b3, float scale, u32 contracts, u32 seats, const uint8_t *__restrict__ seat_sets,
    int4 *__restrict__ value_out, float4 *__restrict__ raw_out, ulonglong2 *__restrict__ feature_words_out) {
    TK_VGPR_TOP(256, 255);
    static_assert(TK_BLOCK == 2 * PM_M && PM_M % 4 == 0 && TK_BID_ROWS == 20 && TK_BID_ROWS <= 64, "two lanes per row, five pieces per row");
    __shared__ __attribute__((aligned(16))) __bf16 X[PM_M * PM_LD];
    __shared__ u64 ext[PM_M][4];
    const int64_t base = (int64_t)blockIdx.x * (PM_M / 4);
    const u32 tid = threadIdx.x, wave = tid >> 6;
    float *L = reinterpret_cast<float *>(X);
    bf16x8 wq[4][2];
    mlp_prefetch(wq, w1, wave * 2);                // lands while the features are built
    if (tid < PM_M) {
        const u32 v = tid & 3u;
        const int64_t gq = base + (tid >> 2), g = gq < n ? gq : n - 1;
        bid_feature_words(deal[(int64_t)v * n + g], v, ext[tid]);
        if (feature_words_out && gq < n) {
            feature_words_out[(g * 4 + v) * 2] = make_ulonglong2(ext[tid][0], ext[tid][1]);
            feature_words_out[(g * 4 + v) * 2 + 1] = make_ulonglong2(ext[tid][2], ext[tid][3]);
        }
    }
    __syncthreads();
    policy_expand(X, ext, tid);
    __syncthreads();
    mlp_hidden(X, w1, b1, wq, wave);
    mlp_prefetch(wq, w2, wave * 2);
    mlp_hidden(X, w2, b2, wq, wave);
    mlp_head(X, L, w3, b3, wave, 0);
    __syncthreads();
    const u32 row = tid >> 1, v = row & 3u;
    const int64_t g = base + (row >> 2);
    if (g >= n) return;
    const u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
    const bool live = ((set >> v) & 1u) && deal[(int64_t)v * n + g] != 0;     // (a valid deal's hand holds twelve cards)
    const u32 rowmask = live ? bid_row_mask(contracts) : 0u;                  // (19 bits: row 19 is never set)
#pragma unroll
    for (u32 p = tid & 1u; p < TK_BID_ROWS / 4; p += 2) {
        const float4 y = *reinterpret_cast<const float4 *>(L + row * PM_LL + 4 * p);
        const float yy[4] = {y.x, y.y, y.z, y.w};
        float rw[4];
        int vl[4];
#pragma unroll
        for (u32 j = 0; j < 4; j++) {
            const bool keep = (rowmask >> (4 * p + j)) & 1u;
            rw[j] = keep ? yy[j] : 0.f;
            vl[j] = keep ? (int)rintf(fminf(fmaxf(yy[j] * scale, -1073741824.f), 1073741824.f)) : 0;
        }
        const int64_t o = (g * 4 + v) * (TK_BID_ROWS / 4) + p;
        if (value_out) value_out[o] = make_int4(vl[0], vl[1], vl[2], vl[3]);
        if (raw_out) raw_out[o] = make_float4(rw[0], rw[1], rw[2], rw[3]);
    }
}

// tarok_bid_values_pass: k_bid_values whose row 19 is output 19, the value of a pass: scaled, clamped and rounded as rows
// 0..18 are, with the same zeros for a seat outside the set and an invalid deal, and whatever `contracts` holds.  A kernel
// of its own, k_bid_values' text with the row mask changed: as one templated body the parent's kernel did not keep its
// instruction count.
__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_bid_values_pass(
    int64_t n, const u64 *__restrict__ deal, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3,
    const float *__restrict__ b3, float scale, u32 contracts, u32 seats, const uint8_t *__restrict__ seat_sets,
    int4 *__restrict__ value_out, float4 *__restrict__ raw_out, ulonglong2 *__restrict__ feature_words_out) {
    TK_VGPR_TOP(256, 255);
    static_assert(TK_BLOCK == 2 * PM_M && PM_M % 4 == 0 && TK_BID_ROWS == 20 && TK_BID_ROWS <= 64, "two lanes per row, five pieces per row");
    __shared__ __attribute__((aligned(16))) __bf16 X[PM_M * PM_LD];
    __shared__ u64 ext[PM_M][4];
    const int64_t base = (int64_t)blockIdx.x * (PM_M / 4);
    const u32 tid = threadIdx.x, wave = tid >> 6;
    float *L = reinterpret_cast<float *>(X);
    bf16x8 wq[4][2];
    mlp_prefetch(wq, w1, wave * 2);                // lands while the features are built
    if (tid < PM_M) {
        const u32 v = tid & 3u;
        const int64_t gq = base + (tid >> 2), g = gq < n ? gq : n - 1;
        bid_feature_words(deal[(int64_t)v * n + g], v, ext[tid]);
        if (feature_words_out && gq < n) {
            feature_words_out[(g * 4 + v) * 2] = make_ulonglong2(ext[tid][0], ext[tid][1]);
            feature_words_out[(g * 4 + v) * 2 + 1] = make_ulonglong2(ext[tid][2], ext[tid][3]);
        }
    }
    __syncthreads();
    policy_expand(X, ext, tid);
    __syncthreads();
    mlp_hidden(X, w1, b1, wq, wave);
    mlp_prefetch(wq, w2, wave * 2);
    mlp_hidden(X, w2, b2, wq, wave);
    mlp_head(X, L, w3, b3, wave, 0);
    __syncthreads();
    const u32 row = tid >> 1, v = row & 3u;
    const int64_t g = base + (row >> 2);
    if (g >= n) return;
    const u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
    const bool live = ((set >> v) & 1u) && deal[(int64_t)v * n + g] != 0;     // (a valid deal's hand holds twelve cards)
    const u32 rowmask = live ? bid_row_mask(contracts) | 1u << TK_BID_PASS_ROW : 0u;      // (row 19 whatever `contracts` holds)
#pragma unroll
    for (u32 p = tid & 1u; p < TK_BID_ROWS / 4; p += 2) {
        const float4 y = *reinterpret_cast<const float4 *>(L + row * PM_LL + 4 * p);
        const float yy[4] = {y.x, y.y, y.z, y.w};
        float rw[4];
        int vl[4];
#pragma unroll
        for (u32 j = 0; j < 4; j++) {
            const bool keep = (rowmask >> (4 * p + j)) & 1u;
            rw[j] = keep ? yy[j] : 0.f;
            vl[j] = keep ? (int)rintf(fminf(fmaxf(yy[j] * scale, -1073741824.f), 1073741824.f)) : 0;
        }
        const int64_t o = (g * 4 + v) * (TK_BID_ROWS / 4) + p;
        if (value_out) value_out[o] = make_int4(vl[0], vl[1], vl[2], vl[3]);
        if (raw_out) raw_out[o] = make_float4(rw[0], rw[1], rw[2], rw[3]);
    }
}

// tarok_exchange_values: the exchange head — k_bid_values' forward on the declarer's pick-up.  A workgroup takes 16 games
// = 128 rows, row = 8 * local game + i, "pick up talon group i": threads below 128 decode their game's 32-byte state and
// build ext[row] = exchange_feature_words(game, i) under w1's prefetch — four zero words for a row that is not live (the
// game does not take part, or i >= ngroups), so ext[row][0] != 0 says "live" to the end of the kernel (word 0 of a live row
// holds the declarer's bit).  After the head the f32 rows in LDS feed the raw_out stores (all 256 threads, 16-byte pieces,
// the workgroup's 32 KiB contiguous), and one thread per game takes the value comparison across the game's rows
// (exchange_choice) and the discards of the winning row (exchange_select on P & TK_DISCARDABLE, the Bot's fallback to
// all of P), or, for a game outside the set, tarok_playout_exchange's other two cases.  A ragged last workgroup's rows
// read game n - 1 and store nothing.  Nothing of the env is written.
__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_exchange_values(
    int64_t n, const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23, const u64 *__restrict__ gkey,
    const __bf16 *__restrict__ w1, const float *__restrict__ b1, const __bf16 *__restrict__ w2, const float *__restrict__ b2,
    const __bf16 *__restrict__ w3, const float *__restrict__ b3, u32 seats, const uint8_t *__restrict__ seat_sets,
    float4 *__restrict__ raw_out, int8_t *__restrict__ choice_out, uint8_t *__restrict__ discards_out,
    ulonglong2 *__restrict__ feature_words_out) {
    TK_VGPR_TOP(256, 255);
    constexpr u32 ROWS = 8, GAMES = PM_M / ROWS;     // rows per game, games per workgroup
    static_assert(TK_BLOCK == 2 * PM_M && PM_M % ROWS == 0 && 64 * PM_M / 4 % TK_BLOCK == 0, "one tile, whole raw pieces per thread");
    __shared__ __attribute__((aligned(16))) __bf16 X[PM_M * PM_LD];
    __shared__ u64 ext[PM_M][4];
    const int64_t base = (int64_t)blockIdx.x * GAMES;
    const u32 tid = threadIdx.x, wave = tid >> 6;
    float *L = reinterpret_cast<float *>(X);
    bf16x8 wq[4][2];
    mlp_prefetch(wq, w1, wave * 2);                // lands while the features are built
    if (tid < PM_M) {
        const u32 i = tid & (ROWS - 1);
        const int64_t gq = base + (tid / ROWS), g = gq < n ? gq : n - 1;
        Game gm;
        load_game(gm, s01, s23, g);
        const u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
        const bool part = gm.phase == TK_PHASE_EXCHANGE && ((set >> gm.declarer) & 1u);
        u64 w[4];
        exchange_feature_words(gm, i, w);
#pragma unroll
        for (u32 j = 0; j < 4; j++) ext[tid][j] = part ? w[j] : 0ULL;
        if (feature_words_out && gq < n) {
            feature_words_out[(g * ROWS + i) * 2] = make_ulonglong2(ext[tid][0], ext[tid][1]);
            feature_words_out[(g * ROWS + i) * 2 + 1] = make_ulonglong2(ext[tid][2], ext[tid][3]);
        }
    }
    __syncthreads();
    policy_expand(X, ext, tid);
    __syncthreads();
    mlp_hidden(X, w1, b1, wq, wave);
    mlp_prefetch(wq, w2, wave * 2);
    mlp_hidden(X, w2, b2, wq, wave);
    mlp_head(X, L, w3, b3, wave, 0);
    __syncthreads();
    if (raw_out) {
#pragma unroll
        for (u32 k = 0; k < 64 * PM_M / 4 / TK_BLOCK; k++) {
            const u32 p = tid + TK_BLOCK * k, row = p >> 4, q = p & 15u;
            if (base + (row / ROWS) < n) {
                const float4 y = *reinterpret_cast<const float4 *>(L + row * PM_LL + 4 * q);
                raw_out[base * (ROWS * 16) + p] = ext[row][0] ? y : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    const int64_t g = base + tid;
    if (tid >= GAMES || g >= n || (!choice_out && !discards_out)) return;
    int ch = -1;
    u32 dpk = 0xFFFFFFu;
    const u64 w0 = ext[tid * ROWS][0];
    if (w0) {                                        // the game takes part: row 0 is live
        const u32 gs = 3u - (u32)__builtin_ctz((u32)(w0 >> 58) & 7u), ngroups = 6u / gs;
        const float *y = L + tid * ROWS * PM_LL;
        ch = (int)exchange_choice(y, PM_LL, ngroups);
        const u64 P = ext[tid * ROWS + (u32)ch][0] & TK_DECK;
        u64 cand = P & TK_DISCARDABLE;
        if ((u32)popc64(cand) < gs) cand = P;
        dpk = exchange_select(y + (u32)ch * PM_LL, cand, gs);
    } else {
        Game gm;
        load_game(gm, s01, s23, g);
        if (gm.phase == TK_PHASE_EXCHANGE) {         // the Bot's own exchange: group 0, its sampler under the game's key
            ch = 0;
            dpk = exchange_discards(gm, 0u, gkey[g]);
        }
    }
    if (choice_out) choice_out[g] = (int8_t)ch;
    if (discards_out) {
        discards_out[g * 3 + 0] = (uint8_t)dpk; discards_out[g * 3 + 1] = (uint8_t)(dpk >> 8);
        discards_out[g * 3 + 2] = (uint8_t)(dpk >> 16);
    }
}

// tarok_exchange_candidates: the discards of every candidate (i, d) of tarok_playout_exchange, one thread per game —
// exchange_discards under that launch's ckey, 255s for groups the contract does not have and for games that do not take
// part.  Read-only; every row written.
TK_KERNEL(TK_BLOCK, 128) void k_exchange_candidates(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 sets, u32 seats,
                                                   const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                                   const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,
                                                   uint8_t *__restrict__ cand_out) {
    TK_VGPR_TOP(128, 127);
    const int64_t g = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (g >= n) return;
    Game g0;
    load_game(g0, s01, s23, g);
    const u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
    const bool part = g0.phase == TK_PHASE_EXCHANGE && ((set >> g0.declarer) & 1u);
    const u32 ngroups = part ? 6u / group_size(g0.contract) : 0u;
    const u64 ebase = (u64)cnt[g].episode << 28;
    uint8_t *out = cand_out + g * (int64_t)(18u * sets);
    for (u32 i = 0; i < 6; i++)
        for (u32 d = 0; d < sets; d++) {
            u32 dpk = 0xFFFFFFu;
            if (i < ngroups) dpk = exchange_discards(g0, i, game_key(pseed, offset + (u64)g, (5ULL << 61) | ebase | ((u64)i << 6) | (u64)d));
            uint8_t *o = out + 3u * (i * sets + d);
            o[0] = (uint8_t)dpk; o[1] = (uint8_t)(dpk >> 8); o[2] = (uint8_t)(dpk >> 16);
        }
}

// tarok_policy_step: tarok_policy_mlp and tarok_step in ONE launch.  A play workgroup (512
// threads, 256 games = the 256 slots of step group blockIdx.x) evaluates the policy for its games
// as two 128-game tiles side by side, leaves the sampled cards in LDS and then runs the step
// kernel's play role on them (threads 0..255; same refill lists, same launch-parity protocol as
// k_play); the workgroups after the play groups run the refill role.
// tarok_policy_step_seats (MIXED) and tarok_policy_step_versus (NETS = 2) are the same launch around another
// instantiation of policy_body; what they take more comes LAST in their kernels' parameters (the set and the per-game
// sets, then the second network's six pointers): the preloaded kernel arguments are the same for the three.
#define TK_POLICY_STEP_ARGS                                                                                                       \
    int64_t n, u64 seed, u64 offset, int mix, int flags, u32 play_groups, u32 *epoch, u32 fan,                                    \
        const u64 *__restrict__ obs_in, const __bf16 *__restrict__ w1, const float *__restrict__ b1,                              \
        const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3,                               \
        const float *__restrict__ b3, uint8_t *__restrict__ action, float *__restrict__ logp, float *__restrict__ value,          \
        ulonglong2 *__restrict__ feature_words_out, int16_t *__restrict__ reward, uint8_t *__restrict__ done,                     \
        uint16_t *__restrict__ trick, u64 *__restrict__ obs_out, uint8_t *__restrict__ hist,                                      \
        ulonglong2 *__restrict__ s01, ulonglong2 *__restrict__ s23, Aux *aux, Counters *__restrict__ cnt,                         \
        u64 *__restrict__ gkey, u64 *rlist, u32 *rcount
#define TK_POLICY_STEP_NAMES                                                                                                      \
    n, seed, offset, mix, flags, play_groups, epoch, fan, obs_in, w1, b1, w2, b2, w3, b3, action, logp, value,                    \
        feature_words_out, reward, done, trick, obs_out, hist, s01, s23, aux, cnt, gkey, rlist, rcount

// `second` (NETS = 2) is the second network's weights, or a callable that gives them: it is called by a play workgroup
// only, after the refill role has branched off (the pool kernels read their group's table entry in it).
__device__ __forceinline__ PolicyWeights second_weights(const PolicyWeights &w) { return w; }
template <class F>
__device__ __forceinline__ PolicyWeights second_weights(const F &f) { return f(); }

template <int NETS, bool MIXED, int MODE = 0, class SECOND = PolicyWeights>
__device__ __forceinline__ void policy_step_shell(TK_POLICY_STEP_ARGS, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                  const SECOND &second, const PlayMode pmode = PlayMode{}) {
    TkCount count = launch_count<1>(epoch, play_groups);          // (in flight under the policy's first loads)
    if (blockIdx.x >= play_groups) {
        refill_role<false>(blockIdx.x - play_groups, threadIdx.x, 2 * TK_BLOCK, seed, offset, mix, play_groups, count, epoch, fan, false, aux, rlist, rcount, nullptr);
        return;
    }
    __shared__ uint8_t act_s[2 * PM_M];
    u32 *lds = nullptr;
    PolicyWeights nets[NETS] = {{w1, b1, w2, b2, w3, b3}};
    if constexpr (NETS > 1) nets[1] = second_weights(second);
    policy_body<2, NETS, MIXED, MODE>(n, s01, s23, obs_in, gkey, nets, action, logp, value, nullptr, feature_words_out, nullptr, act_s, &lds,
                                      seats, seat_sets, pmode);
    __syncthreads();                          // (the policy's LDS is free from here on: the step's scoring list goes there)
    u32 tid = threadIdx.x;
    step_role<false, false>(blockIdx.x, tid & (TK_BLOCK - 1), tid < TK_BLOCK, act_s[tid & (TK_BLOCK - 1)], false, n, seed, offset, mix, flags,
                           count, epoch, play_groups, fan, nullptr, nullptr, reward, done, trick, obs_out, hist, s01, s23, aux, cnt, gkey, rlist, rcount, nullptr,
                           reinterpret_cast<u32 (*)[TK_BLOCK]>(lds));
}

__global__ __launch_bounds__(2 * TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_policy_step(TK_POLICY_STEP_ARGS) {
    TK_VGPR_TOP(256, 255);
    policy_step_shell<1, false>(TK_POLICY_STEP_NAMES, 15, nullptr, PolicyWeights{});
}

__global__ __launch_bounds__(2 * TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_policy_step_seats(
    TK_POLICY_STEP_ARGS, u32 seats, const uint8_t *__restrict__ seat_sets) {
    TK_VGPR_TOP(256, 255);
    policy_step_shell<1, true>(TK_POLICY_STEP_NAMES, seats, seat_sets, PolicyWeights{});
}

__global__ __launch_bounds__(2 * TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_policy_step_versus(
    TK_POLICY_STEP_ARGS, u32 seats, const uint8_t *__restrict__ seat_sets, const __bf16 *__restrict__ v1,
    const float *__restrict__ c1, const __bf16 *__restrict__ v2, const float *__restrict__ c2, const __bf16 *__restrict__ v3,
    const float *__restrict__ c3) {
    TK_VGPR_TOP(256, 255);
    policy_step_shell<2, false>(TK_POLICY_STEP_NAMES, seats, seat_sets, PolicyWeights{v1, c1, v2, c2, v3, c3});
}

// The same three launches under a play mode (MODE = 1): the mode's four values come LAST, after whatever the kind takes.
#define TK_PLAY_MODE_ARGS float inv_t, int greedy, u32 thr, float eps
#define TK_PLAY_MODE_NAMES PlayMode{inv_t, greedy, thr, eps}
__global__ __launch_bounds__(2 * TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_policy_step_mode(TK_POLICY_STEP_ARGS, TK_PLAY_MODE_ARGS) {
    TK_VGPR_TOP(256, 255);
    policy_step_shell<1, false, 1>(TK_POLICY_STEP_NAMES, 15, nullptr, PolicyWeights{}, TK_PLAY_MODE_NAMES);
}

__global__ __launch_bounds__(2 * TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_policy_step_seats_mode(
    TK_POLICY_STEP_ARGS, u32 seats, const uint8_t *__restrict__ seat_sets, TK_PLAY_MODE_ARGS) {
    TK_VGPR_TOP(256, 255);
    policy_step_shell<1, true, 1>(TK_POLICY_STEP_NAMES, seats, seat_sets, PolicyWeights{}, TK_PLAY_MODE_NAMES);
}

__global__ __launch_bounds__(2 * TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_policy_step_versus_mode(
    TK_POLICY_STEP_ARGS, u32 seats, const uint8_t *__restrict__ seat_sets, const __bf16 *__restrict__ v1,
    const float *__restrict__ c1, const __bf16 *__restrict__ v2, const float *__restrict__ c2, const __bf16 *__restrict__ v3,
    const float *__restrict__ c3, TK_PLAY_MODE_ARGS) {
    TK_VGPR_TOP(256, 255);
    policy_step_shell<2, false, 1>(TK_POLICY_STEP_NAMES, seats, seat_sets, PolicyWeights{v1, c1, v2, c2, v3, c3}, TK_PLAY_MODE_NAMES);
}

// tarok_policy_step_pool: k_policy_step_versus whose second network is chosen PER PLAY WORKGROUP (= step group) from a
// pool of pool_size networks, six stacked arrays with entry k at base + k * size.  The group's index k is
// group_net[blockIdx.x], or blockIdx.x % pool_size without a table; k >= pool_size is the learner's own network (nets[1]
// = nets[0]: plain self-play for the group, and no read outside the pool whatever the byte).  k is workgroup-uniform and
// made so in the compiler's eyes (readfirstlane): the weights stay on scalar base registers, the tiles, the LDS and the
// order of accumulation are the versus kernel's.  What the kind takes more comes last, as for the other kinds; a refill
// workgroup never reads group_net.
#define TK_POOL_ARGS                                                                                                              \
    u32 pool_size, const __bf16 *__restrict__ p1, const float *__restrict__ q1, const __bf16 *__restrict__ p2,                    \
        const float *__restrict__ q2, const __bf16 *__restrict__ p3, const float *__restrict__ q3,                                \
        const uint8_t *__restrict__ group_net
#define TK_POOL_SECOND                                                                                                            \
    [&]() __attribute__((always_inline)) {                                                                                        \
        u32 k = group_net ? (u32)group_net[blockIdx.x] : blockIdx.x % pool_size;                                                  \
        k = (u32)__builtin_amdgcn_readfirstlane((int)k);                                                                          \
        if (k >= pool_size) return PolicyWeights{w1, b1, w2, b2, w3, b3};                                                         \
        return PolicyWeights{p1 + (size_t)k * 65536, q1 + (size_t)k * 256, p2 + (size_t)k * 65536, q2 + (size_t)k * 256,          \
                             p3 + (size_t)k * 16384, q3 + (size_t)k * 64};                                                        \
    }
__global__ __launch_bounds__(2 * TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_policy_step_pool(
    TK_POLICY_STEP_ARGS, u32 seats, const uint8_t *__restrict__ seat_sets, TK_POOL_ARGS) {
    TK_VGPR_TOP(256, 255);
    policy_step_shell<2, false>(TK_POLICY_STEP_NAMES, seats, seat_sets, TK_POOL_SECOND);
}

__global__ __launch_bounds__(2 * TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_policy_step_pool_mode(
    TK_POLICY_STEP_ARGS, u32 seats, const uint8_t *__restrict__ seat_sets, TK_POOL_ARGS, TK_PLAY_MODE_ARGS) {
    TK_VGPR_TOP(256, 255);
    policy_step_shell<2, false, 1>(TK_POLICY_STEP_NAMES, seats, seat_sets, TK_POOL_SECOND, TK_PLAY_MODE_NAMES);
}
#undef TK_POOL_SECOND
#undef TK_POOL_ARGS

// ---------------------------------------------------------------------------
// tarok_playout_cards_net: tarok_playout_cards_det at one playout per (legal card, world), whose playouts are played by a
// policy network on the seats of `net_seats` and by the Bot on the others.  Three launches on one stream
// over the caller's scratch, one ITEM per (game, rank j, world w), item = (g * 12 + j) * worlds + w, four arrays:
//   i01, i23 [items] the item's 32 state bytes (a live item's only), ikey [items] its playout key (a live item's only),
//   ires [items] TK_PN_LIVE while the item is to be played, else its four final scores, packed (0: no such item).
// No score is -32768, so TK_PN_LIVE is no result.
#define TK_PN_LIVE 0x8000800080008000ULL
#define TK_PN_ITEM_BYTES 48
#define TK_PN_MAX_CARDS 48

// First launch: the card launches' worlds (playout_cards_body's team layout, dealers and keys: the dealer's Record in
// LDS, its per-game word, Dealer::deal under the world key), the candidate card applied, the items written.  An item whose
// candidate ends the game is written finished; the slots of absent ranks and of games that do not take part get 0.  A
// hidden world's item is the packed Game whose C plane and talon ids moved: the second launch unpacks all of it.
// VIEWER (tarok_playout_cards_net_value): a live item's marker carries the viewer — the seat to move in the env's position —
// in its two low bits (lane 0 is -32768 + viewer: no score is near).
// SAMPLED (tarok_playout_cards_net_sampled): `samples` items per (rank, world), numbered by net_sampled_slot
// (tarok_device.h); a world's samples load the same world slot — the team's layout stays sized by `worlds` — and sample k's
// key is the item key with k in its ten low bits, the pkey of playout_cards_body.  Without it `samples` is not read.
template <class Dealer, bool VIEWER = false, bool SAMPLED = false>
__device__ __forceinline__ void playout_net_deal_body(int64_t n, u64 pseed, u64 offset, u32 worlds, u32 lg, u32 seats,
                                                      const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                                      const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,
                                                      const typename Dealer::Extra *__restrict__ extra, ulonglong2 *__restrict__ i01,
                                                      ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey, u64 *__restrict__ ires,
                                                      u32 samples = 1) {
    __shared__ typename Dealer::Record world;
    const PlayoutTeam t(lg, worlds);
    const int64_t g = t.g;
    ulonglong2 a = {0, 0}, b = {0, 0};
    CardPosition p;
    u64 ebase = 0;
    u32 nlegal = 0;
    if (g < n) {
        a = s01[g]; b = s23[g];
        Game g0;
        unpack(g0, a.x, a.y, b.x, b.y);
        p = card_position(g0, seat_sets, seats, g);
        if (p.takes_part) {
            nlegal = (u32)popc64(p.legal);
            ebase = ((u64)cnt[g].episode << 28) | ((u64)p.played << 22);
            const typename Dealer::Extra word = game_word(extra, g);
            for (u32 w = t.lane; w < worlds; w += t.L) {
                Game d = g0;
                Dealer::deal(d, p.mover, game_key(pseed, offset + (u64)g, Dealer::world_tag | ebase | (u64)w), word);
                world.store(t.slot0 + w, d);
            }
        }
    }
    __syncthreads();
    if (g < n) {
        const u32 slots = SAMPLED ? net_sampled_slots(worlds, samples) : TAROK_PLAYOUT_RANKS * worlds;
        for (u32 i = t.lane; i < slots; i += t.L) {
            const int64_t it = g * (int64_t)slots + i;
            u32 j = i / worlds, w = i - j * worlds, k = 0;
            if constexpr (SAMPLED) net_sampled_split(i, worlds, samples, j, w, k);
            u64 res = 0;
            if (j < nlegal) {                            // (nlegal = 0 for a game that does not take part)
                const u32 c = kth_bit(p.legal, j);
                Game h;
                unpack(h, a.x, a.y, b.x, b.y);
                world.load(t.slot0 + w, h);
                u64 scores = 0;
                u32 ti;
                const int fin = apply_step<true>(h, c, scores, ti, false);
                res = fin ? scores : (VIEWER ? TK_PN_LIVE | (u64)p.mover : TK_PN_LIVE);
                if (!fin) {
                    u64 x0, x1, y0, y1;
                    pack(h, x0, x1, y0, y1);
                    i01[it] = make_ulonglong2(x0, x1);
                    i23[it] = make_ulonglong2(y0, y1);
                    ikey[it] = game_key(pseed, offset + (u64)g, Dealer::item_tag | ebase | ((u64)c << 16) | ((u64)w << 10) | (u64)k);
                }
            }
            ires[it] = res;
        }
    }
}

// The six first launches, one per dealer with and without the viewer in a live item's marker (tarok_playout_cards_net_value's).
// WORDS: the body's words argument; after it the kernel's own words parameter, which a det kernel does not have.
//   k_playout_net_deal         redeal_unseen's worlds
//   k_playout_net_deal_voids   the worlds honour shown voids (redeal_voids under voids[g], as k_playout_voids)
//   k_playout_net_deal_hidden  the worlds also re-deal Klop's talon and the declarer's discards (redeal_hidden under played[g],
//                              as k_playout_hidden; WorldABCT slots: 36 bytes x TK_PO_WORLD_SLOTS = 2,304 bytes of LDS)
#define TK_NET_DEAL(NAME, DEALER, VIEWER, WORDS, ...)                                                                              \
    TK_KERNEL(TK_BLOCK, 128) void NAME(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 worlds, u32 lg, u32 seats,           \
                                      const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,                    \
                                      const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt, __VA_ARGS__             \
                                      ulonglong2 *__restrict__ i01, ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey,           \
                                      u64 *__restrict__ ires) {                                                                     \
        TK_VGPR_TOP(128, 127);                                                                                                      \
        playout_net_deal_body<DEALER, VIEWER>(n, pseed, offset, worlds, lg, seats, seat_sets, s01, s23, cnt, WORDS, i01, i23, ikey, \
                                              ires);                                                                                \
    }
TK_NET_DEAL(k_playout_net_deal, DealUnseen, false, nullptr, )
TK_NET_DEAL(k_playout_net_deal_voids, DealVoids, false, voids, const u32 *__restrict__ voids, )
TK_NET_DEAL(k_playout_net_deal_hidden, DealHidden, false, played_words, const u64 *__restrict__ played_words, )
TK_NET_DEAL(k_playout_net_deal_value, DealUnseen, true, nullptr, )
TK_NET_DEAL(k_playout_net_deal_value_voids, DealVoids, true, voids, const u32 *__restrict__ voids, )
TK_NET_DEAL(k_playout_net_deal_value_hidden, DealHidden, true, played_words, const u64 *__restrict__ played_words, )
#undef TK_NET_DEAL

// tarok_playout_cards_net_sampled's first launches: the three VIEWER dealers over (rank, world, sample) items; `samples` comes
// last, after the item arrays.
#define TK_NET_DEAL_SAMPLED(NAME, DEALER, WORDS, ...)                                                                              \
    TK_KERNEL(TK_BLOCK, 128) void NAME(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 worlds, u32 lg, u32 seats,           \
                                      const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,                    \
                                      const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt, __VA_ARGS__             \
                                      ulonglong2 *__restrict__ i01, ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey,           \
                                      u64 *__restrict__ ires, u32 samples) {                                                        \
        TK_VGPR_TOP(128, 127);                                                                                                      \
        playout_net_deal_body<DEALER, true, true>(n, pseed, offset, worlds, lg, seats, seat_sets, s01, s23, cnt, WORDS, i01, i23,   \
                                                  ikey, ires, samples);                                                             \
    }
TK_NET_DEAL_SAMPLED(k_playout_net_deal_sampled, DealUnseen, nullptr, )
TK_NET_DEAL_SAMPLED(k_playout_net_deal_sampled_voids, DealVoids, voids, const u32 *__restrict__ voids, )
TK_NET_DEAL_SAMPLED(k_playout_net_deal_sampled_hidden, DealHidden, played_words, const u64 *__restrict__ played_words, )
#undef TK_NET_DEAL_SAMPLED

// Second launch: the playouts.  A workgroup of 256 threads keeps one tile of PM_M = 128 items resident — their packed
// states and keys in LDS, owned by threads 0..127 — and plays them card by card: feature words (policy_feature_words on
// the item's own Game) -> policy_expand, mlp_hidden x 2, mlp_head, unchanged, so a row's logits are tarok_policy_mlp's
// bits -> the greedy card of policy_sample<1> (two lanes per row) into act_s, or the Bot's card policy_action(key, q,
// legal) for a seat outside net_seats -> apply_step<true>.  The forward is skipped in a card round in which no live
// row's mover is a net seat.  LDS: X 67,584 + ext 4,096 + states 4,096 + keys 1,024 + cards and votes < 77 KB, two
// workgroups per CU as k_policy_mlp, so one's integer work runs under the other's MFMAs.
//
// LOOP INVARIANTS (the card loop has workgroup barriers inside it):
//   - the continuation test and the forward test read vote[parity][0..1], written by waves 0 and 1 before the round's
//     first barrier and read by every thread after it: both are workgroup-uniform.  Two parities, because a round
//     without a forward has no other barrier between this read and the next round's write;
//   - the loop runs at most TK_PN_MAX_CARDS = 48 rounds (a game has 48 cards), whatever the items hold;
//   - a live row with an empty legal mask is retired with result 0, not waited for;
//   - a workgroup whose items are all dead leaves at the first round's test: it runs no forward;
//   - a row still live after the last round (none can be) gets result 0: TK_PN_LIVE never reaches the third launch.
//
// VALUE (k_playout_net_play_value, tarok_playout_cards_net_value): a live item's marker carries its viewer
// in the two low bits, and the owning thread counts down `depth` at every position with the viewer to move.  The row
// that reaches 0 STOPS in that round: it plays no card, writes rint(clamp(v54 * value_scale)) into the viewer's column
// (zeros in the other three) and dies.  What changes in the invariants above, and nothing else:
//   - a THIRD vote bit (4): some live row stops this round.  It is written with the other two by waves 0 and 1 before
//     the round's first barrier, so the forward test `v & 6` is workgroup-uniform as `v & 2` is; the two parities stay,
//     and no barrier moved into a divergent branch;
//   - the value reaches the owning thread as the card does: val_s[row], written next to act_s[row] by the row's
//     half == 0 lane between the forward's last two barriers (512 bytes more LDS: 77,456 in all, still two per CU);
//   - a stopping row is retired in its round whatever its legal mask holds; depth = TAROK_PLAYOUT_MAX_DEPTH never counts
//     to 0 (a seat has at most 11 cards after its candidate), and every round is then the plain kernel's.
//
// VERSUS (k_playout_net_play_versus*, tarok_playout_cards_net_versus): two networks, seated RELATIVE to each
// item's viewer (net_versus_role, tarok_device.h); net_seats is not read.  A live item's marker always carries its viewer
// (the caller's item kernel is the _value form also at depth 0).  What changes in the invariants above, and nothing else:
//   - waves 0 and 1 write each row's role (0 Bot, 1 A, 2 B; bit 2: the row stops this round) to role_s[row], the second
//     half of act_s, before the round's first barrier;
//   - vote bit 2 means "some live row needs a pass of A", and a FOURTH bit (8) "some live row needs a pass of B": a row
//     that plays a card needs its role's pass, a row that stops needs its viewer's network's pass alone.  Both are written
//     with the first before the round's first barrier, so the pass tests are workgroup-uniform; the two parities stay;
//   - the forward runs once per set pass bit — X re-expanded from ext each time, the third barrier of a pass keeps the
//     next pass's expansion off the logits being read — and in pass P a row's half == 0 lane writes act_s only where the
//     row's role is P, val_s only where the row stops and P is the viewer's network.  No barrier is in a divergent branch.
//
// MODE = 1 (k_playout_net_play_sampled*, tarok_playout_cards_net_sampled; under VERSUS only): a network seat
// plays what the table's sampler gives under ITS network's PlayMode — ma for role A, mb for role B — with the item's key and
// the row's cards played q: the tempered draw (or the greedy card), and the Bot's card where the mode's coin says explore.
// What changes in the invariants above, and nothing else:
//   - waves 0 and 1 write each row's q to q_s[row], the third part of act_s, with its role, before the round's first
//     barrier (0 for a dead row); the votes, the two parities, the 48 rounds and the pass tests are VERSUS';
//   - in pass P the sampler runs with P's mode, picked by scalar selects on the pass number like the weight pointers, on
//     in.key = keys[row], in.played = q_s[row] and in.last as policy_sample_inputs sets it.  EVERY thread runs it whatever
//     its row's role: policy_sample's partner reads (pm_swap) — the greedy ones and MODE's — are all inside it, none
//     in a select or a branch here;
//   - the exploring card replaces the drawn one on the half == 0 lane, which holds the whole pick, before act_s is
//     written; the value read for a stop is untouched by the mode.  No barrier is added.
template <bool VALUE, bool VERSUS = false, int MODE = 0>
__device__ __forceinline__ void playout_net_play_body(int64_t items, u32 net_seats, u32 depth, float value_scale,
                                                      const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
                                                      const u64 *__restrict__ ikey, u64 *__restrict__ ires,
                                                      const __bf16 *__restrict__ w1, const float *__restrict__ b1,
                                                      const __bf16 *__restrict__ w2, const float *__restrict__ b2,
                                                      const __bf16 *__restrict__ w3, const float *__restrict__ b3,
                                                      u32 own_rel = 0, u32 opp_rel = 0, const PolicyWeights &wb = PolicyWeights{},
                                                      const PlayMode &ma = PlayMode{}, const PlayMode &mb = PlayMode{}) {
    static_assert(!MODE || VERSUS, "a play mode per network is the VERSUS body's");
    constexpr bool MARKED = VALUE || VERSUS;             // a live item's marker carries its viewer
    __shared__ __attribute__((aligned(16))) __bf16 X[PM_M * PM_LD];
    __shared__ __attribute__((aligned(16))) u64 ext[PM_M][4];
    __shared__ __attribute__((aligned(16))) u64 st[PM_M][4];
    __shared__ u64 keys[PM_M];
    __shared__ uint8_t act_s[MODE ? 3 * PM_M : VERSUS ? 2 * PM_M : PM_M];
    __shared__ u32 vote[2][2];
    __shared__ float val_s[VALUE ? PM_M : 1];
    uint8_t *role_s = act_s + (VERSUS ? PM_M : 0);       // (VERSUS only)
    uint8_t *q_s = act_s + (MODE ? 2 * PM_M : 0);        // (MODE only)
    const u32 tid = threadIdx.x, wave = tid >> 6;
    const int64_t it = (int64_t)blockIdx.x * PM_M + tid;
    float *L = reinterpret_cast<float *>(X);
    bool live = false;
    u32 viewer = 0, left = depth;
    u64 mark = 0;
    if (tid < PM_M && it < items && ((mark = ires[it]) & (MARKED ? ~3ULL : ~0ULL)) == TK_PN_LIVE) {
        live = true;
        if constexpr (MARKED) viewer = (u32)mark & 3u;
        const ulonglong2 a = i01[it], b = i23[it];
        st[tid][0] = a.x; st[tid][1] = a.y; st[tid][2] = b.x; st[tid][3] = b.y;
        keys[tid] = ikey[it];
    }
#pragma unroll 1
    for (u32 round = 0; round < TK_PN_MAX_CARDS; round++) {
        bool stop = false;
        u32 role = 0;                                      // (VERSUS only: the mover's, kept by the row's owner)
        if (tid < PM_M) {                                  // (waves 0 and 1, whole)
            bool net = false, net_b = false;               // (VERSUS: the row needs a pass of A / of B)
            if (live) {
                Game h;
                unpack(h, st[tid][0], st[tid][1], st[tid][2], st[tid][3]);
                policy_feature_words(h, ext[tid]);
                if constexpr (VERSUS) {
                    const u32 mover = (h.leader + h.nt) & 3;
                    role = net_versus_role(viewer, mover, own_rel, opp_rel);
                    if constexpr (VALUE) {
                        if (mover == viewer) stop = --left == 0;
                    }
                    const u32 need = stop ? net_versus_viewer_net(opp_rel) : role;
                    net = need == 1u; net_b = need == 2u;
                    role_s[tid] = (uint8_t)(role | (stop ? 4u : 0u));
                    if constexpr (MODE) q_s[tid] = (uint8_t)(h.trick_no * 4 + h.nt);
                } else {
                    net = (net_seats >> ((h.leader + h.nt) & 3)) & 1u;
                    if constexpr (VALUE) {
                        if (((h.leader + h.nt) & 3) == viewer) stop = --left == 0;
                    }
                }
            } else {
                ext[tid][0] = 0; ext[tid][1] = 0; ext[tid][2] = 0; ext[tid][3] = 0;
                if constexpr (VERSUS) role_s[tid] = 0;
                if constexpr (MODE) q_s[tid] = 0;
            }
            const u64 any_live = __ballot(live), any_net = __ballot(live && net);
            if constexpr (VERSUS) {
                const u64 any_b = __ballot(live && net_b); // (every lane of the wave is here: tid < PM_M takes whole waves)
                if (__lane_id() == 0) vote[round & 1][wave] = (any_live ? 1u : 0u) | (any_net ? 2u : 0u) | (any_b ? 8u : 0u);
            } else if constexpr (VALUE) {
                const u64 any_stop = __ballot(stop);       // (every lane of the wave is here: tid < PM_M takes whole waves)
                if (__lane_id() == 0) vote[round & 1][wave] = (any_live ? 1u : 0u) | (any_net ? 2u : 0u) | (any_stop ? 4u : 0u);
            } else {
                if (__lane_id() == 0) vote[round & 1][wave] = (any_live ? 1u : 0u) | (any_net ? 2u : 0u);
            }
        }
        __syncthreads();
        const u32 v = vote[round & 1][0] | vote[round & 1][1];
        if (!(v & 1u)) break;
        if constexpr (VERSUS) {
            const u32 viewer_net = net_versus_viewer_net(opp_rel);
#pragma unroll 1
            for (u32 pass = 1; pass <= 2; pass++) {        // (v is the workgroup's: every thread runs the same passes)
                if (!(v & (pass == 1 ? 2u : 8u))) continue;
                const bool pa = pass == 1;
                const __bf16 *p1 = pa ? w1 : wb.w1, *p2 = pa ? w2 : wb.w2, *p3 = pa ? w3 : wb.w3;
                const float *c1 = pa ? b1 : wb.b1, *c2 = pa ? b2 : wb.b2, *c3 = pa ? b3 : wb.b3;
                bf16x8 wq[4][2];
                mlp_prefetch(wq, p1, wave * 2);
                policy_expand(X, ext, tid);
                __syncthreads();
                mlp_hidden(X, p1, c1, wq, wave);
                mlp_prefetch(wq, p2, wave * 2);
                mlp_hidden(X, p2, c2, wq, wave);
                mlp_head(X, L, p3, c3, wave, 0);
                __syncthreads();
                const u32 gi = tid >> 1, half = tid & 1;
                PolicySampleIn in;
                in.m = ext[gi][1] & TAROK_OBS_MASK;
                in.o = in.m; in.key = 0; in.played = 0; in.last = 0;
                in.mh = (u32)(in.m >> (27 * half)) & 0x7FFFFFFu;
                PlayMode pm = PlayMode{1.f, 1, 0u, 0.f};
                if constexpr (MODE) {
                    pm = PlayMode{pa ? ma.inv_t : mb.inv_t, pa ? ma.greedy : mb.greedy, pa ? ma.thr : mb.thr, pa ? ma.eps : mb.eps};
                    in.key = keys[gi]; in.played = q_s[gi];
                    in.last = in.m ? 63 - __clzll(in.m) : 0;
                }
                PolicyPick c = policy_sample<1>(L, gi, half, in, pm);
                if (half == 0) {
                    const u32 rs = role_s[gi];
                    if constexpr (MODE) {                  // the mode's coin: an exploring seat plays the Bot's card of the position
                        if (in.m && pm.thr && (rng32(in.key, TK_DRAW_EXPLORE + in.played) >> 8) < pm.thr) c.pk = c.bc;
                    }
                    if ((rs & 3u) == pass) act_s[gi] = (uint8_t)c.pk;
                    if constexpr (VALUE) {
                        if ((rs & 4u) && viewer_net == pass) val_s[gi] = c.v54;
                    }
                }
                __syncthreads();
            }
        } else if (v & (VALUE ? 6u : 2u)) {
            bf16x8 wq[4][2];
            mlp_prefetch(wq, w1, wave * 2);
            policy_expand(X, ext, tid);
            __syncthreads();
            mlp_hidden(X, w1, b1, wq, wave);
            mlp_prefetch(wq, w2, wave * 2);
            mlp_hidden(X, w2, b2, wq, wave);
            mlp_head(X, L, w3, b3, wave, 0);
            __syncthreads();
            // the greedy card of row gi, two lanes per row: policy_sample<1> under a greedy mode (its draw, its exps and
            // the Bot's card are not read: they fold away)
            const u32 gi = tid >> 1, half = tid & 1;
            PolicySampleIn in;
            in.m = ext[gi][1] & TAROK_OBS_MASK;
            in.o = in.m; in.key = 0; in.played = 0; in.last = 0;
            in.mh = (u32)(in.m >> (27 * half)) & 0x7FFFFFFu;
            const PolicyPick c = policy_sample<1>(L, gi, half, in, PlayMode{1.f, 1, 0u, 0.f});
            if (half == 0) {
                act_s[gi] = (uint8_t)c.pk;
                if constexpr (VALUE) val_s[gi] = c.v54;
            }
            __syncthreads();
        }
        if (live) {
            Game h;
            unpack(h, st[tid][0], st[tid][1], st[tid][2], st[tid][3]);
            const u64 legal = ext[tid][1] & TAROK_OBS_MASK;
            if (VALUE && stop) {                           // the viewer's depth-th decision: the value head's estimate, no card
                float t = val_s[tid] * value_scale;
                t = t != t ? 0.f : t;
                t = fminf(fmaxf(t, -32767.f), 32767.f);
                live = false;
                ires[it] = (u64)(uint16_t)(int)rintf(t) << (16 * viewer);
            } else if (!legal) {
                live = false;
                ires[it] = 0;
            } else {
                const u32 seat = (h.leader + h.nt) & 3, q = h.trick_no * 4 + h.nt;
                const bool by_net = VERSUS ? role != 0u : ((net_seats >> seat) & 1u) != 0u;
                const u32 c = by_net ? (u32)act_s[tid] : policy_action(keys[tid], q, legal);
                u64 scores = 0;
                u32 ti;
                if (apply_step<true>(h, c, scores, ti, false)) {
                    live = false;
                    ires[it] = scores;
                } else {
                    pack(h, st[tid][0], st[tid][1], st[tid][2], st[tid][3]);
                }
            }
        }
    }
    if (live) ires[it] = 0;
}

__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_playout_net_play(
    int64_t items, u32 net_seats, const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
    const u64 *__restrict__ ikey, u64 *__restrict__ ires, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3, const float *__restrict__ b3) {
    TK_VGPR_TOP(256, 255);
    playout_net_play_body<false>(items, net_seats, 0, 0.f, i01, i23, ikey, ires, w1, b1, w2, b2, w3, b3);
}

// tarok_playout_cards_net_value's second launch: what the kind takes more comes last, as for the other kinds.
__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_playout_net_play_value(
    int64_t items, u32 net_seats, const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
    const u64 *__restrict__ ikey, u64 *__restrict__ ires, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3, const float *__restrict__ b3,
    u32 depth, float value_scale) {
    TK_VGPR_TOP(256, 255);
    playout_net_play_body<true>(items, net_seats, depth, value_scale, i01, i23, ikey, ires, w1, b1, w2, b2, w3, b3);
}

// tarok_playout_cards_net_versus' second launch: the VERSUS body over the dense count, network A as the six arrays every
// play kernel takes, then the two role sets and network B; the _value form stops at the viewer's depth-th decision.
__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_playout_net_play_versus(
    int64_t items, u32 own_rel, const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
    const u64 *__restrict__ ikey, u64 *__restrict__ ires, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3, const float *__restrict__ b3,
    u32 opp_rel, PolicyWeights wb) {
    TK_VGPR_TOP(256, 255);
    playout_net_play_body<false, true>(items, 0, 0, 0.f, i01, i23, ikey, ires, w1, b1, w2, b2, w3, b3, own_rel, opp_rel, wb);
}

__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_playout_net_play_versus_value(
    int64_t items, u32 own_rel, const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
    const u64 *__restrict__ ikey, u64 *__restrict__ ires, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3, const float *__restrict__ b3,
    u32 opp_rel, PolicyWeights wb, u32 depth, float value_scale) {
    TK_VGPR_TOP(256, 255);
    playout_net_play_body<true, true>(items, 0, depth, value_scale, i01, i23, ikey, ires, w1, b1, w2, b2, w3, b3, own_rel, opp_rel, wb);
}

// tarok_playout_cards_net_sampled's second launch: the VERSUS body under a play mode per network (MODE = 1); the two modes come
// after network B, each as tarok_set_play_mode converts it.
#define TK_PLAY_MODES_ARGS float inv_t_a, int greedy_a, u32 thr_a, float eps_a, float inv_t_b, int greedy_b, u32 thr_b, float eps_b
#define TK_PLAY_MODES_NAMES PlayMode{inv_t_a, greedy_a, thr_a, eps_a}, PlayMode{inv_t_b, greedy_b, thr_b, eps_b}
__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_playout_net_play_sampled(
    int64_t items, u32 own_rel, const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
    const u64 *__restrict__ ikey, u64 *__restrict__ ires, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3, const float *__restrict__ b3,
    u32 opp_rel, PolicyWeights wb, TK_PLAY_MODES_ARGS) {
    TK_VGPR_TOP(256, 255);
    playout_net_play_body<false, true, 1>(items, 0, 0, 0.f, i01, i23, ikey, ires, w1, b1, w2, b2, w3, b3, own_rel, opp_rel, wb,
                                          TK_PLAY_MODES_NAMES);
}

__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_playout_net_play_sampled_value(
    int64_t items, u32 own_rel, const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
    const u64 *__restrict__ ikey, u64 *__restrict__ ires, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3, const float *__restrict__ b3,
    u32 opp_rel, PolicyWeights wb, TK_PLAY_MODES_ARGS, u32 depth, float value_scale) {
    TK_VGPR_TOP(256, 255);
    playout_net_play_body<true, true, 1>(items, 0, depth, value_scale, i01, i23, ikey, ires, w1, b1, w2, b2, w3, b3, own_rel, opp_rel, wb,
                                         TK_PLAY_MODES_NAMES);
}
#undef TK_PLAY_MODES_NAMES
#undef TK_PLAY_MODES_ARGS

// Third launch: 16 lanes per game; lane r < 12 sums rank r's items over the worlds in integers, then card_epilogue's
// write-out on the game's position, as the det launch.
TK_KERNEL(TK_BLOCK, 64) void k_playout_net_sum(int64_t n, u32 worlds, u32 seats, const uint8_t *__restrict__ seat_sets,
                                              const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                              const u64 *__restrict__ gkey, const u64 *__restrict__ ires,
                                              int4 *__restrict__ sum_out, uint8_t *__restrict__ action_out) {
    TK_VGPR_TOP(64, 63);
    __shared__ __attribute__((aligned(16))) int sums[(TK_BLOCK >> 4) * TAROK_PLAYOUT_RANKS * 4];
    const PlayoutTeam t(4);
    int *row = sums + t.team * (TAROK_PLAYOUT_RANKS * 4);
    CardPosition p;
    u32 nlegal = 0;
    if (t.g < n) {
        Game g0;
        load_game(g0, s01, s23, t.g);
        p = card_position(g0, seat_sets, seats, t.g);
        if (p.takes_part) nlegal = (u32)popc64(p.legal);
        if (t.lane < TAROK_PLAYOUT_RANKS) {
            const u64 *r = ires + (t.g * TAROK_PLAYOUT_RANKS + t.lane) * (int64_t)worlds;
            int4 s = make_int4(0, 0, 0, 0);
            for (u32 w = 0; w < worlds; w++) {
                const u64 sc = r[w];
                s.x += (int)(int16_t)sc; s.y += (int)(int16_t)(sc >> 16); s.z += (int)(int16_t)(sc >> 32); s.w += (int)(int16_t)(sc >> 48);
            }
            reinterpret_cast<int4 *>(row)[t.lane] = s;
        }
    }
    __syncthreads();
    if (t.g < n) card_epilogue(t, row, p, nlegal, gkey, sum_out, action_out);
}

// ---------------------------------------------------------------------------
// tarok_playout_cards_net_halving: the net card launch with sequential halving on a COMPACTED item list.
// Per game three words live in the scratch across the rounds — alive[g] (the ranks alive), on[g] (the ranks that play the
// round: alive, or 0 for a game that does not take part or is down to one card after round 0) and base[g] (the game's first
// item of the round: the exclusive prefix sum of net_list_count(on, W_r)) — beside its running [12][4] sums and [12]
// counts.  A round is: the scan (three launches: no workgroup waits on another), the items, the playouts
// (playout_net_play_body on the round's total, read from a device word), the sums and the survivor rule.  One stream, no
// host read: the item arrays are sized by the host's bound n * a_r * W_r (net_list_bound).

// k_playout_net_list_init: 16 lanes a game, as k_playout_net_sum: zero running sums and counts, alive and round 0's on.
TK_KERNEL(TK_BLOCK, 64) void k_playout_net_list_init(int64_t n, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                    const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                                    u32 *__restrict__ on, u32 *__restrict__ alive, int4 *__restrict__ rsum,
                                                    int4 *__restrict__ rcnt) {
    TK_VGPR_TOP(64, 63);
    const PlayoutTeam t(4);
    if (t.g >= n) return;
    if (t.lane < TAROK_PLAYOUT_RANKS) rsum[t.g * TAROK_PLAYOUT_RANKS + t.lane] = make_int4(0, 0, 0, 0);
    else if (t.lane < TAROK_PLAYOUT_RANKS + 3u) rcnt[t.g * 3 + (t.lane - TAROK_PLAYOUT_RANKS)] = make_int4(0, 0, 0, 0);
    else if (t.lane == 15u) {
        Game g0;
        load_game(g0, s01, s23, t.g);
        const CardPosition p = card_position(g0, seat_sets, seats, t.g);
        const u32 a = p.takes_part ? (1u << (u32)popc64(p.legal)) - 1u : 0u;
        alive[t.g] = a;
        on[t.g] = a;
    }
}

// The exclusive prefix sum of one value a thread over the workgroup's TK_BLOCK threads (Hillis-Steele in LDS; every thread
// of the workgroup calls it) -> the sum of the values below the thread's; `total`: the workgroup's sum.
__device__ __forceinline__ u32 block_exclusive_scan(u32 v, u32 *lds /* [TK_BLOCK] */, u32 &total) {
    const u32 tid = threadIdx.x;
    u32 x = v;
    lds[tid] = x;
    __syncthreads();
#pragma unroll
    for (u32 d = 1; d < TK_BLOCK; d <<= 1) {
        const u32 y = tid >= d ? lds[tid - d] : 0u;
        __syncthreads();
        x += y;
        lds[tid] = x;
        __syncthreads();
    }
    total = lds[TK_BLOCK - 1];
    __syncthreads();                                     // (the caller may scan again over the same words)
    return x - v;
}

// The scan's first launch: a workgroup of TK_BLOCK games -> part[block], its items of the round.
TK_KERNEL(TK_BLOCK, 64) void k_playout_net_list_totals(int64_t n, u32 round_worlds, const u32 *__restrict__ on, u32 *__restrict__ part) {
    TK_VGPR_TOP(64, 63);
    __shared__ u32 lds[TK_BLOCK];
    const int64_t g = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    u32 total;
    block_exclusive_scan(g < n ? net_list_count(on[g], round_worlds) : 0u, lds, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// The second: ONE workgroup turns part[0 .. blocks - 1] into its exclusive prefix sums, TK_BLOCK words a pass with the
// carry in a register, and writes the round's total.
TK_KERNEL(TK_BLOCK, 64) void k_playout_net_list_scan(u32 blocks, u32 *__restrict__ part, u32 *__restrict__ total_out) {
    TK_VGPR_TOP(64, 63);
    __shared__ u32 lds[TK_BLOCK];
    u32 carry = 0;
    for (u32 b0 = 0; b0 < blocks; b0 += TK_BLOCK) {      // (launch-uniform: every thread meets the same barriers)
        const u32 i = b0 + threadIdx.x;
        u32 total;
        const u32 x = block_exclusive_scan(i < blocks ? part[i] : 0u, lds, total);
        if (i < blocks) part[i] = carry + x;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// The third: base[g] = the items of the workgroups before the game's + those of the games before it in its own.
TK_KERNEL(TK_BLOCK, 64) void k_playout_net_list_base(int64_t n, u32 round_worlds, const u32 *__restrict__ on, const u32 *__restrict__ part,
                                                    u32 *__restrict__ base) {
    TK_VGPR_TOP(64, 63);
    __shared__ u32 lds[TK_BLOCK];
    const int64_t g = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    u32 total;
    const u32 x = block_exclusive_scan(g < n ? net_list_count(on[g], round_worlds) : 0u, lds, total);
    if (g < n) base[g] = part[blockIdx.x] + x;
}

// The round's items: playout_net_deal_body's team, dealer, keys and item words, for the ranks of on[g] in the round's worlds
// e0 .. e0 + round_worlds - 1 alone — the team deals only those, into its world slots 0 .. round_worlds - 1, under their true
// indices — each written to its compact slot net_list_slot(base[g], q, round_worlds, w - e0).  A game's items are
// net_list_count(on[g]) <= a_r * round_worlds, so every slot written lies below the round's total and below the host's bound.
template <class Dealer, bool VIEWER>
__device__ __forceinline__ void playout_net_list_deal_body(int64_t n, u64 pseed, u64 offset, u32 e0, u32 round_worlds, u32 lg, u32 seats,
                                                           const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                                           const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,
                                                           const typename Dealer::Extra *__restrict__ extra, const u32 *__restrict__ on,
                                                           const u32 *__restrict__ base, ulonglong2 *__restrict__ i01,
                                                           ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey, u64 *__restrict__ ires) {
    __shared__ typename Dealer::Record world;
    const PlayoutTeam t(lg, round_worlds);
    const int64_t g = t.g;
    ulonglong2 a = {0, 0}, b = {0, 0};
    CardPosition p;
    u64 ebase = 0;
    u32 o = 0, first = 0;
    if (g < n && (o = on[g]) != 0u) {                    // (on: only games that take part)
        first = base[g];
        a = s01[g]; b = s23[g];
        Game g0;
        unpack(g0, a.x, a.y, b.x, b.y);
        p = card_position(g0, seat_sets, seats, g);
        ebase = ((u64)cnt[g].episode << 28) | ((u64)p.played << 22);
        const typename Dealer::Extra word = game_word(extra, g);
        for (u32 lw = t.lane; lw < round_worlds; lw += t.L) {
            Game d = g0;
            Dealer::deal(d, p.mover, game_key(pseed, offset + (u64)g, Dealer::world_tag | ebase | (u64)(e0 + lw)), word);
            world.store(t.slot0 + lw, d);
        }
    }
    __syncthreads();
    const u32 count = net_list_count(o, round_worlds);
    for (u32 i = t.lane; i < count; i += t.L) {
        const u32 q = i / round_worlds, lw = i - q * round_worlds, w = e0 + lw;
        const u32 it = net_list_slot(first, q, round_worlds, lw);
        const u32 c = kth_bit(p.legal, kth_bit_word(o, 0u, q));
        Game h;
        unpack(h, a.x, a.y, b.x, b.y);
        world.load(t.slot0 + lw, h);
        u64 scores = 0;
        u32 ti;
        const int fin = apply_step<true>(h, c, scores, ti, false);
        if (!fin) {
            u64 x0, x1, y0, y1;
            pack(h, x0, x1, y0, y1);
            i01[it] = make_ulonglong2(x0, x1);
            i23[it] = make_ulonglong2(y0, y1);
            ikey[it] = game_key(pseed, offset + (u64)g, Dealer::item_tag | ebase | ((u64)c << 16) | ((u64)w << 10));
        }
        ires[it] = fin ? scores : (VIEWER ? TK_PN_LIVE | (u64)p.mover : TK_PN_LIVE);
    }
}

#define TK_NET_LIST_DEAL(NAME, DEALER, VIEWER, WORDS_T)                                                                            \
    TK_KERNEL(TK_BLOCK, 128) void NAME(int64_t n, u64 pseed /* seed ^ salt */, u64 offset, u32 e0, u32 round_worlds, u32 lg,        \
                                      u32 seats, const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,         \
                                      const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,                         \
                                      const WORDS_T *__restrict__ words, const u32 *__restrict__ on, const u32 *__restrict__ base,  \
                                      ulonglong2 *__restrict__ i01, ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey,           \
                                      u64 *__restrict__ ires) {                                                                     \
        TK_VGPR_TOP(128, 127);                                                                                                      \
        playout_net_list_deal_body<DEALER, VIEWER>(n, pseed, offset, e0, round_worlds, lg, seats, seat_sets, s01, s23, cnt, words,  \
                                                   on, base, i01, i23, ikey, ires);                                                 \
    }
TK_NET_LIST_DEAL(k_playout_net_list_deal, DealUnseen, false, NoWord)                  // words: nullptr
TK_NET_LIST_DEAL(k_playout_net_list_deal_voids, DealVoids, false, u32)
TK_NET_LIST_DEAL(k_playout_net_list_deal_hidden, DealHidden, false, u64)
TK_NET_LIST_DEAL(k_playout_net_list_deal_value, DealUnseen, true, NoWord)
TK_NET_LIST_DEAL(k_playout_net_list_deal_value_voids, DealVoids, true, u32)
TK_NET_LIST_DEAL(k_playout_net_list_deal_value_hidden, DealHidden, true, u64)
#undef TK_NET_LIST_DEAL

// The round's playouts: k_playout_net_play / _value on the round's total, which no host knows — the grid is the bound's, and a
// workgroup past the total has no live row and leaves at the first round's vote (playout_net_play_body's invariants).
__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_playout_net_play_list(
    const u32 *__restrict__ total, u32 net_seats, const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
    const u64 *__restrict__ ikey, u64 *__restrict__ ires, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3, const float *__restrict__ b3) {
    TK_VGPR_TOP(256, 255);
    playout_net_play_body<false>((int64_t)*total, net_seats, 0, 0.f, i01, i23, ikey, ires, w1, b1, w2, b2, w3, b3);
}

__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_playout_net_play_list_value(
    const u32 *__restrict__ total, u32 net_seats, const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
    const u64 *__restrict__ ikey, u64 *__restrict__ ires, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3, const float *__restrict__ b3,
    u32 depth, float value_scale) {
    TK_VGPR_TOP(256, 255);
    playout_net_play_body<true>((int64_t)*total, net_seats, depth, value_scale, i01, i23, ikey, ires, w1, b1, w2, b2, w3, b3);
}

// tarok_playout_cards_net_versus_halving's playouts: the VERSUS body on the round's total.
__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_playout_net_play_list_versus(
    const u32 *__restrict__ total, u32 own_rel, const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
    const u64 *__restrict__ ikey, u64 *__restrict__ ires, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3, const float *__restrict__ b3,
    u32 opp_rel, PolicyWeights wb) {
    TK_VGPR_TOP(256, 255);
    playout_net_play_body<false, true>((int64_t)*total, 0, 0, 0.f, i01, i23, ikey, ires, w1, b1, w2, b2, w3, b3, own_rel, opp_rel, wb);
}

__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_playout_net_play_list_versus_value(
    const u32 *__restrict__ total, u32 own_rel, const ulonglong2 *__restrict__ i01, const ulonglong2 *__restrict__ i23,
    const u64 *__restrict__ ikey, u64 *__restrict__ ires, const __bf16 *__restrict__ w1, const float *__restrict__ b1,
    const __bf16 *__restrict__ w2, const float *__restrict__ b2, const __bf16 *__restrict__ w3, const float *__restrict__ b3,
    u32 opp_rel, PolicyWeights wb, u32 depth, float value_scale) {
    TK_VGPR_TOP(256, 255);
    playout_net_play_body<true, true>((int64_t)*total, 0, depth, value_scale, i01, i23, ikey, ires, w1, b1, w2, b2, w3, b3, own_rel, opp_rel,
                                      wb);
}

// The round's sums and the survivor rule: 16 lanes a game, as k_playout_net_sum.  Lane j < 12 whose rank played the round adds
// its round_worlds results, in integers, to the game's running sums and sets the rank's count to the round's end e1; the
// team's block in LDS is playout_halving_body's ([12][4] sums, [12] counts).  After the barrier: not the last round ->
// halve_alive on the mover's column, the new alive[g] and the next round's on[g]; the last -> the launch's three outputs,
// the card by best_alive over the ranks alive, the Bot's for a game in play that does not take part.
TK_KERNEL(TK_BLOCK, 128) void k_playout_net_list_sum(int64_t n, u32 e1, u32 round_worlds, u32 last, u32 seats,
                                                    const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                                    const ulonglong2 *__restrict__ s23, const u64 *__restrict__ gkey,
                                                    const u64 *__restrict__ ires, u32 *__restrict__ on, u32 *__restrict__ alive,
                                                    const u32 *__restrict__ base, int4 *__restrict__ rsum, int *__restrict__ rcnt,
                                                    int4 *__restrict__ sum_out, int4 *__restrict__ count_out,
                                                    uint8_t *__restrict__ action_out) {
    TK_VGPR_TOP(128, 127);
    constexpr u32 INTS = TAROK_PLAYOUT_RANKS * 5;
    __shared__ __attribute__((aligned(16))) int sums[(TK_BLOCK >> 4) * INTS];
    const PlayoutTeam t(4);
    const int64_t g = t.g;
    int *row = sums + t.team * INTS;
    u32 o = 0, al = 0;
    if (g < n) {
        o = on[g]; al = alive[g];
        if (t.lane < TAROK_PLAYOUT_RANKS) {
            const u32 j = t.lane;
            int4 s = rsum[g * TAROK_PLAYOUT_RANKS + j];
            int c = rcnt[g * TAROK_PLAYOUT_RANKS + j];
            if ((o >> j) & 1u) {
                const u64 *r = ires + net_list_slot(base[g], (u32)__popc(o & ((1u << j) - 1u)), round_worlds, 0u);
                for (u32 w = 0; w < round_worlds; w++) {
                    const u64 sc = r[w];
                    s.x += (int)(int16_t)sc; s.y += (int)(int16_t)(sc >> 16); s.z += (int)(int16_t)(sc >> 32); s.w += (int)(int16_t)(sc >> 48);
                }
                c = (int)e1;
                rsum[g * TAROK_PLAYOUT_RANKS + j] = s;
                rcnt[g * TAROK_PLAYOUT_RANKS + j] = c;
            }
            reinterpret_cast<int4 *>(row)[j] = s;
            row[TAROK_PLAYOUT_RANKS * 4 + j] = c;
        }
    }
    __syncthreads();
    if (g >= n) return;
    if (last) {
        if (sum_out && t.lane < TAROK_PLAYOUT_RANKS) sum_out[g * TAROK_PLAYOUT_RANKS + t.lane] = reinterpret_cast<const int4 *>(row)[t.lane];
        if (count_out && t.lane >= 12u && t.lane < 15u)
            count_out[g * 3 + (t.lane - 12u)] = reinterpret_cast<const int4 *>(row)[TAROK_PLAYOUT_RANKS + (t.lane - 12u)];
    }
    if (t.lane != 15u || (last && !action_out)) return;
    Game g0;
    load_game(g0, s01, s23, g);
    const CardPosition p = card_position(g0, seat_sets, seats, g);
    if (!last) {
        const u32 next = halve_alive(row, al, p.mover);
        alive[g] = next;
        on[g] = (next & (next - 1u)) != 0u ? next : 0u;     // a game down to one card plays no further round
    } else {
        u32 act = 255;
        if (p.takes_part) act = kth_bit(p.legal, best_alive(row, al, p.mover));
        else if (p.in_play) act = policy_action(gkey[g], p.played, p.legal);
        action_out[g] = (uint8_t)act;
    }
}

// ---------------------------------------------------------------------------
// tarok_playout_exchange_net / tarok_playout_bids_net: the exchange and the bid valued by playouts that
// k_playout_net_play plays.  An exchange candidate in a world, or a bid option in a world, is an item at 0 cards played
// under the key the Bot launch uses at sample 0; the scratch holds the four item arrays of tarok_playout_cards_net.

// What decides whether a game takes part in an exchange launch, for both of its kernels.
struct ExchangePosition {
    u32 declarer = 0, ncand = 0;
    bool waiting = false, takes_part = false;
};
__device__ __forceinline__ ExchangePosition exchange_position(const Game &g0, const uint8_t *__restrict__ seat_sets, u32 seats, u32 sets,
                                                              int64_t g) {
    ExchangePosition p;
    p.waiting = g0.phase == TK_PHASE_EXCHANGE;
    p.declarer = g0.declarer;
    if (p.waiting) {
        u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
        p.takes_part = (set >> p.declarer) & 1u;
    }
    if (p.takes_part) {
        const u32 gs = group_size(g0.contract);
        p.ncand = (gs == 3 ? 2u : (gs == 2 ? 3u : 6u)) * sets;
    }
    return p;
}

// Exchange, first launch: the front half of k_playout_exchange — its team layout, worlds, candidates and keys — and, where
// that kernel plays an item, the game after apply_exchange packed and written with the item's key (k = 0) and TK_PN_LIVE.
// Item (g * 6 * sets + r) * worlds + w; a row at or beyond ncand, or a game that takes no part, gets result 0 and
// nothing else.  VIEWER (tarok_playout_exchange_net_value's first launch): a live item's marker also carries
// the declarer, the seat the candidates are valued for, as playout_net_deal_body<Dealer, true> writes the mover.
template <bool VIEWER>
__device__ __forceinline__ void playout_exchange_net_deal_body(int64_t n, int64_t items, u64 pseed, u64 offset, u32 worlds, u32 sets, u32 lg,
                                                               u32 seats, const uint8_t *__restrict__ seat_sets,
                                                               const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                                               const Counters *__restrict__ cnt, ulonglong2 *__restrict__ i01,
                                                               ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey, u64 *__restrict__ ires) {
    __shared__ WorldAB world;
    __shared__ u32 cand_dpk[(TK_BLOCK >> TK_PX_MIN_LG) * TK_PX_ROWS];
    const PlayoutTeam t(lg, worlds);
    const u32 L = t.L, lane = t.lane;
    const int64_t g = t.g;
    u32 *cand = cand_dpk + t.team * TK_PX_ROWS;
    ulonglong2 a = {0, 0}, b = {0, 0};
    u64 ebase = 0;
    ExchangePosition p;
    if (g < n) {
        a = s01[g]; b = s23[g];
        Game g0;
        unpack(g0, a.x, a.y, b.x, b.y);
        p = exchange_position(g0, seat_sets, seats, sets, g);
        if (p.takes_part) {
            ebase = (u64)cnt[g].episode << 28;
            for (u32 w = lane; w < worlds; w += L) {
                Game d = g0;
                redeal_unseen(d, p.declarer, game_key(pseed, offset + (u64)g, (7ULL << 61) | ebase | (63ULL << 22) | (u64)w));
                world.store(t.slot0 + w, d);
            }
            for (u32 r = lane; r < p.ncand; r += L) {
                u32 i = r / sets, d = r - i * sets;
                cand[r] = exchange_discards(g0, i, game_key(pseed, offset + (u64)g, (5ULL << 61) | ebase | ((u64)i << 6) | (u64)d));
            }
        }
    }
    __syncthreads();
    if (g >= n) return;
    const u32 slots = 6u * sets * worlds;
    for (u32 s = lane; s < slots; s += L) {
        const int64_t it = g * (int64_t)slots + s;
        if (it >= items) break;
        const u32 r = s / worlds, w = s - r * worlds;
        u64 res = 0;
        if (r < p.ncand) {                               // (ncand = 0 for a game that does not take part)
            const u32 i = r / sets, d = r - i * sets;
            Game h;
            unpack(h, a.x, a.y, b.x, b.y);
            world.load(t.slot0 + w, h);
            const u32 dpk = cand[r];
            apply_exchange(h, i, dpk & 255, (dpk >> 8) & 255, (dpk >> 16) & 255);
            u64 x0, x1, y0, y1;
            pack(h, x0, x1, y0, y1);
            i01[it] = make_ulonglong2(x0, x1);
            i23[it] = make_ulonglong2(y0, y1);
            ikey[it] = game_key(pseed, offset + (u64)g, (3ULL << 62) | ebase | (63ULL << 22) | ((u64)(8u * i + d) << 16) | ((u64)w << 10));
            res = VIEWER ? TK_PN_LIVE | (u64)p.declarer : TK_PN_LIVE;
        }
        ires[it] = res;
    }
}

#define TK_EXCHANGE_NET_DEAL(NAME, VIEWER)                                                                                            \
    TK_KERNEL(TK_BLOCK, 128) void NAME(int64_t n, int64_t items, u64 pseed /* seed ^ salt */, u64 offset, u32 worlds, u32 sets,       \
                                      u32 lg, u32 seats, const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,   \
                                      const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,                           \
                                      ulonglong2 *__restrict__ i01, ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey,             \
                                      u64 *__restrict__ ires) {                                                                       \
        TK_VGPR_TOP(128, 127);                                                                                                        \
        playout_exchange_net_deal_body<VIEWER>(n, items, pseed, offset, worlds, sets, lg, seats, seat_sets, s01, s23, cnt, i01, i23,  \
                                               ikey, ires);                                                                           \
    }
TK_EXCHANGE_NET_DEAL(k_playout_exchange_net_deal, false)
TK_EXCHANGE_NET_DEAL(k_playout_exchange_net_deal_value, true)
#undef TK_EXCHANGE_NET_DEAL

// Exchange, third launch: 16 lanes per game; lane r, r + 16, r + 32 sum their rows' items over the worlds in integers,
// then the tail of k_playout_exchange: 6 * sets 16-byte rows, and on lane 0 the choice — the first candidate at the
// maximum of the declarer's sums with its discards drawn again under the candidate key, the Bot's own exchange for a
// waiting game outside the set, -1 and 255s elsewhere.
TK_KERNEL(TK_BLOCK, 64) void k_playout_exchange_net_sum(int64_t n, int64_t items, u64 pseed /* seed ^ salt */, u64 offset, u32 worlds,
                                                       u32 sets, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                       const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                                       const Counters *__restrict__ cnt, const u64 *__restrict__ gkey,
                                                       const u64 *__restrict__ ires, int4 *__restrict__ sum_out,
                                                       int8_t *__restrict__ choice_out, uint8_t *__restrict__ discards_out) {
    TK_VGPR_TOP(64, 63);
    __shared__ __attribute__((aligned(16))) int sums[(TK_BLOCK >> 4) * TK_PX_ROWS * 4];
    const PlayoutTeam t(4);
    const int64_t g = t.g;
    int *row = sums + t.team * (TK_PX_ROWS * 4);
    const u32 nrows = 6u * sets;
    if (g < n) {
        for (u32 r = t.lane; r < nrows; r += t.L) {
            const int64_t first = (g * (int64_t)nrows + r) * (int64_t)worlds;
            int4 s = make_int4(0, 0, 0, 0);
            for (u32 w = 0; w < worlds; w++) {
                const u64 sc = first + w < items ? ires[first + w] : 0ULL;
                s.x += (int)(int16_t)sc; s.y += (int)(int16_t)(sc >> 16); s.z += (int)(int16_t)(sc >> 32); s.w += (int)(int16_t)(sc >> 48);
            }
            reinterpret_cast<int4 *>(row)[r] = s;
        }
    }
    __syncthreads();
    if (g >= n) return;
    if (sum_out)
        for (u32 r = t.lane; r < nrows; r += t.L) sum_out[g * nrows + r] = reinterpret_cast<const int4 *>(row)[r];
    if ((choice_out || discards_out) && t.lane == 0) {
        Game g0;
        load_game(g0, s01, s23, g);
        const ExchangePosition p = exchange_position(g0, seat_sets, seats, sets, g);
        int ch = -1;
        u32 dpk = 0xFFFFFFu;
        if (p.takes_part) {                              // the first candidate at the maximum of the declarer's sums
            const u32 best = best_row(row, p.ncand, p.declarer), i = best / sets, d = best - i * sets;
            ch = (int)i;
            dpk = exchange_discards(g0, i, game_key(pseed, offset + (u64)g, (5ULL << 61) | ((u64)cnt[g].episode << 28) | ((u64)i << 6) | (u64)d));
        } else if (p.waiting) {                          // the Bot's own exchange: group 0, its sampler under the game's key
            ch = 0;
            dpk = exchange_discards(g0, 0u, gkey[g]);
        }
        if (choice_out) choice_out[g] = (int8_t)ch;
        if (discards_out) {
            discards_out[g * 3 + 0] = (uint8_t)dpk; discards_out[g * 3 + 1] = (uint8_t)(dpk >> 8);
            discards_out[g * 3 + 2] = (uint8_t)(dpk >> 16);
        }
    }
}

// Bids, second launch (after k_bid_deal): k_playout_bids' viewer loop — its team layout, worlds and keys, its barriers
// outside every test of the seat set — writing items where that kernel plays them: bid_game, the Bot's exchange under the
// item's key (k = 0) where the contract has one, the game packed with the key and TK_PN_LIVE.  Item ((g * 4 + v) *
// TAROK_BID_ROWS + r) * worlds + w; the slots of rows outside `contracts` (row 19 among them), of viewers outside the set
// and of invalid deal rows get result 0 and nothing else.
TK_KERNEL(TK_BLOCK, 128) void k_playout_bids_net_deal(int64_t n, int64_t items, u64 pseed /* seed ^ salt */, u64 offset, u32 episode,
                                                     u32 worlds, u32 lg, u32 contracts, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                     const u64 *__restrict__ deal, ulonglong2 *__restrict__ i01,
                                                     ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey, u64 *__restrict__ ires) {
    TK_VGPR_TOP(128, 127);
    __shared__ u64 world_a[TK_PO_WORLD_SLOTS], world_b[TK_PO_WORLD_SLOTS], world_ids[TK_PO_WORLD_SLOTS];
    const PlayoutTeam t(lg, worlds);
    const u32 L = t.L, lane = t.lane, slot0 = t.slot0;
    const int64_t g = t.g;
    u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, tal = 0;
    u32 set = 0;
    if (g < n) {
        h0 = deal[g]; h1 = deal[n + g]; h2 = deal[2 * n + g]; h3 = deal[3 * n + g]; tal = deal[4 * n + g];
        set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
        if ((h0 | h1 | h2 | h3) == 0) set = 0;           // an invalid deal row
    }
    const u32 rowmask = bid_row_mask(contracts), slots = (u32)TAROK_BID_ROWS * worlds;
    const u64 ebase = (u64)episode << 28;
#pragma unroll 1
    for (u32 v = 0; v < 4; v++) {
        const bool part = (set >> v) & 1u;
        __syncthreads();                                 // the last viewer's items have read their worlds
        if (part) {
            for (u32 w = lane; w < worlds; w += L) {
                u64 A, B, ids;
                bid_world(h0, h1, h2, h3, tal, v, game_key(pseed, offset + (u64)g, (2ULL << 61) | ebase | ((u64)v << 6) | (u64)w), A, B, ids);
                world_a[slot0 + w] = A; world_b[slot0 + w] = B; world_ids[slot0 + w] = ids;
            }
        }
        __syncthreads();
        if (g < n) {
            for (u32 s = lane; s < slots; s += L) {
                const int64_t it = (g * 4 + (int64_t)v) * (int64_t)slots + s;
                if (it >= items) break;
                const u32 r = s / worlds, w = s - r * worlds;
                u64 res = 0;
                if (part && ((rowmask >> r) & 1u)) {
                    const u64 pkey = game_key(pseed, offset + (u64)g, (3ULL << 61) | ebase | ((u64)v << 26) | ((u64)r << 21) | ((u64)w << 15));
                    Game h;
                    bid_game(h, world_a[slot0 + w], world_b[slot0 + w], world_ids[slot0 + w], r, v);
                    if (h.phase == TK_PHASE_EXCHANGE) bot_exchange(h, pkey);
                    u64 x0, x1, y0, y1;
                    pack(h, x0, x1, y0, y1);
                    i01[it] = make_ulonglong2(x0, x1);
                    i23[it] = make_ulonglong2(y0, y1);
                    ikey[it] = pkey;
                    res = TK_PN_LIVE;
                }
                ires[it] = res;
            }
        }
    }
}

// tarok_playout_bids_net_value's second launch, text of its own — as one templated body the kernel above
// compiled to other instructions than its parent's: the kernel above with the VIEWER in a live item's marker — v, the seat
// whose row it is, in its two low bits — in the Klop row too, where seat 0 declares.  PASS: slot (g, v, 19, w) is a live
// item as well, k_playout_bids_pass's item under that launch's key with r = 19 and k = 0: pass_round's contract, declarer
// and king set up on the world by bid_game_as, then the Bot's exchange where the game has one; its viewer is v, whoever
// declares.  The viewer loop's two barriers per viewer stand outside every test of the seat set, as in the kernel above.
template <bool PASS>
__device__ __forceinline__ void playout_bids_net_deal_value_body(int64_t n, int64_t items, u64 pseed, u64 offset, u32 episode, u32 worlds, u32 lg,
                                                           u32 contracts, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                           const u64 *__restrict__ deal, ulonglong2 *__restrict__ i01,
                                                           ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey, u64 *__restrict__ ires) {
    __shared__ u64 world_a[TK_PO_WORLD_SLOTS], world_b[TK_PO_WORLD_SLOTS], world_ids[TK_PO_WORLD_SLOTS];
    const PlayoutTeam t(lg, worlds);
    const u32 L = t.L, lane = t.lane, slot0 = t.slot0;
    const int64_t g = t.g;
    u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, tal = 0;
    u32 set = 0;
    if (g < n) {
        h0 = deal[g]; h1 = deal[n + g]; h2 = deal[2 * n + g]; h3 = deal[3 * n + g]; tal = deal[4 * n + g];
        set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
        if ((h0 | h1 | h2 | h3) == 0) set = 0;           // an invalid deal row
    }
    const u32 rowmask = bid_row_mask(contracts), slots = (u32)TAROK_BID_ROWS * worlds;
    const u64 ebase = (u64)episode << 28;
#pragma unroll 1
    for (u32 v = 0; v < 4; v++) {
        const bool part = (set >> v) & 1u;
        __syncthreads();                                 // the last viewer's items have read their worlds
        if (part) {
            for (u32 w = lane; w < worlds; w += L) {
                u64 A, B, ids;
                bid_world(h0, h1, h2, h3, tal, v, game_key(pseed, offset + (u64)g, (2ULL << 61) | ebase | ((u64)v << 6) | (u64)w), A, B, ids);
                world_a[slot0 + w] = A; world_b[slot0 + w] = B; world_ids[slot0 + w] = ids;
            }
        }
        __syncthreads();
        if (g < n) {
            for (u32 s = lane; s < slots; s += L) {
                const int64_t it = (g * 4 + (int64_t)v) * (int64_t)slots + s;
                if (it >= items) break;
                const u32 r = s / worlds, w = s - r * worlds;
                u64 res = 0;
                if (part && (((rowmask >> r) & 1u) || (PASS && r == (u32)TK_BID_PASS_ROW))) {
                    const u64 pkey = game_key(pseed, offset + (u64)g, (3ULL << 61) | ebase | ((u64)v << 26) | ((u64)r << 21) | ((u64)w << 15));
                    Game h;
                    if constexpr (PASS) {                // (k_playout_bids_pass's one setup for both kinds of item)
                        u32 ct = bid_row_contract(r), d = ct == TK_KLOP ? 0u : v, kg = bid_row_king(r);
                        if (r == (u32)TK_BID_PASS_ROW) pass_round(pkey, v, ct, d, kg);
                        bid_game_as(h, world_a[slot0 + w], world_b[slot0 + w], world_ids[slot0 + w], ct, d, kg);
                    } else {
                        bid_game(h, world_a[slot0 + w], world_b[slot0 + w], world_ids[slot0 + w], r, v);
                    }
                    if (h.phase == TK_PHASE_EXCHANGE) bot_exchange(h, pkey);
                    u64 x0, x1, y0, y1;
                    pack(h, x0, x1, y0, y1);
                    i01[it] = make_ulonglong2(x0, x1);
                    i23[it] = make_ulonglong2(y0, y1);
                    ikey[it] = pkey;
                    res = TK_PN_LIVE | (u64)v;
                }
                ires[it] = res;
            }
        }
    }
}

#define TK_BIDS_NET_DEAL_ARGS                                                                                                          \
    int64_t n, int64_t items, u64 pseed /* seed ^ salt */, u64 offset, u32 episode, u32 worlds, u32 lg, u32 contracts, u32 seats,    \
        const uint8_t *__restrict__ seat_sets, const u64 *__restrict__ deal, ulonglong2 *__restrict__ i01, ulonglong2 *__restrict__ i23, \
        u64 *__restrict__ ikey, u64 *__restrict__ ires
#define TK_BIDS_NET_DEAL_NAMES n, items, pseed, offset, episode, worlds, lg, contracts, seats, seat_sets, deal, i01, i23, ikey, ires
// tarok_playout_bids_net_value's second launch, without and with the pass item: two forms, not a launch argument, so the
// launch without the pass carries no bidding round (DESIGN §8.19 has the instruction counts).
TK_KERNEL(TK_BLOCK, 128) void k_playout_bids_net_deal_value(TK_BIDS_NET_DEAL_ARGS) {
    TK_VGPR_TOP(128, 127);
    playout_bids_net_deal_value_body<false>(TK_BIDS_NET_DEAL_NAMES);
}

TK_KERNEL(TK_BLOCK, 128) void k_playout_bids_net_deal_value_pass(TK_BIDS_NET_DEAL_ARGS) {
    TK_VGPR_TOP(128, 127);
    playout_bids_net_deal_value_body<true>(TK_BIDS_NET_DEAL_NAMES);
}
#undef TK_BIDS_NET_DEAL_NAMES
#undef TK_BIDS_NET_DEAL_ARGS

// Bids, fourth launch: one thread per (game, viewer, row); the VIEWER's 16 bits of the result words of its items,
// summed over the worlds in integers.  Row 19 and every slot that held no item sum zeros.
TK_KERNEL(TK_BLOCK, 64) void k_playout_bids_net_sum(int64_t rows /* n * 4 * TAROK_BID_ROWS */, int64_t items, u32 worlds,
                                                   const u64 *__restrict__ ires, int *__restrict__ sum_out) {
    TK_VGPR_TOP(64, 63);
    const int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= rows) return;
    const u32 v = (u32)((i / TAROK_BID_ROWS) & 3);
    const int64_t first = i * (int64_t)worlds;
    int s = 0;
    for (u32 w = 0; w < worlds; w++) {
        const u64 sc = first + w < items ? ires[first + w] : 0ULL;
        s += (int)(int16_t)(sc >> (16 * v));
    }
    sum_out[i] = s;
}

// ---------------------------------------------------------------------------
// tarok_playout_exchange_net_list / tarok_playout_bids_net_list: the two launches above on a COMPACTED item
// list, §8.21's: a UNIT — (game, talon group) for the exchange, (game, viewer) for the bids — has an `on` word of its live
// rows (exchange_list_on / bid_list_on, tarok_device.h) and, from k_playout_net_list_totals / _scan / _base run over the
// units, a first slot base[u]; the item of the q-th set bit in world w is net_list_slot(base[u], q, worlds, w).  The deal
// kernels are the dense kernels' teams, worlds, candidates, barriers and keys looping over live rows only; every slot they
// write is tested against the host's bound, and every slot below the list's total is written.  As k_playout_net_list_deal*
// they take the first world e0 and the count round_worlds, and serve §8.23's rounds too: this launch is e0 = 0 over all its
// worlds (launch_exchange_list_deal / launch_bids_list_deal pick the kernel for both).

// Exchange, first launch: one thread a unit.
TK_KERNEL(TK_BLOCK, 64) void k_playout_exchange_net_list_init(int64_t units, u32 sets, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                             const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                                             u32 *__restrict__ on) {
    TK_VGPR_TOP(64, 63);
    const int64_t u = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (u >= units) return;
    const int64_t g = u / 6;
    Game g0;
    load_game(g0, s01, s23, g);
    const ExchangePosition p = exchange_position(g0, seat_sets, seats, sets, g);
    on[u] = exchange_list_on(g0.contract, (u32)(u - g * 6), sets, p.takes_part);
}

// Exchange, the items, for the list launch and for every halving round (§8.23): playout_exchange_net_deal_body's team, barrier,
// keys and candidates (VIEWER: its marker) over live rows only.  The team deals the worlds e0 + lw, lw < round_worlds, into its
// world slots 0 .. round_worlds - 1, and row r = i * sets + d of a unit whose bit d is on goes to the slot of the bit's rank in
// the word.  A game's items are popc(its on words) * round_worlds, so every slot written lies below the launch's total and
// below the host's bound (tested all the same).  The list launch is e0 = 0, round_worlds = worlds, on the init kernel's words:
//  - a game plays if any of its six on words is non-zero; exchange_list_on makes that exchange_position's takes_part, since a
//    game that takes part has ncand > 0 and so group 0 on;
//  - a list word is the low `sets` bits or 0, so the rank of its bit d is d.
template <bool VIEWER>
__device__ __forceinline__ void playout_exchange_net_list_deal_body(int64_t n, u32 bound, u64 pseed, u64 offset, u32 e0, u32 round_worlds,
                                                                    u32 sets, u32 lg, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                                    const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                                                    const Counters *__restrict__ cnt, const u32 *__restrict__ on,
                                                                    const u32 *__restrict__ base, ulonglong2 *__restrict__ i01,
                                                                    ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey,
                                                                    u64 *__restrict__ ires) {
    __shared__ WorldAB world;
    __shared__ u32 cand_dpk[(TK_BLOCK >> TK_PX_MIN_LG) * TK_PX_ROWS];
    const PlayoutTeam t(lg, round_worlds);
    const u32 L = t.L, lane = t.lane;
    const int64_t g = t.g;
    u32 *cand = cand_dpk + t.team * TK_PX_ROWS;
    ulonglong2 a = {0, 0}, b = {0, 0};
    u64 ebase = 0;
    ExchangePosition p;
    bool plays = false;
    if (g < n) {
        for (u32 i = 0; i < 6; i++) plays = plays || on[g * 6 + i] != 0u;      // (on: only games that take part)
        if (plays) {
            a = s01[g]; b = s23[g];
            Game g0;
            unpack(g0, a.x, a.y, b.x, b.y);
            p = exchange_position(g0, seat_sets, seats, sets, g);
            ebase = (u64)cnt[g].episode << 28;
            for (u32 lw = lane; lw < round_worlds; lw += L) {
                Game d = g0;
                redeal_unseen(d, p.declarer, game_key(pseed, offset + (u64)g, (7ULL << 61) | ebase | (63ULL << 22) | (u64)(e0 + lw)));
                world.store(t.slot0 + lw, d);
            }
            for (u32 r = lane; r < p.ncand; r += L) {
                u32 i = r / sets, d = r - i * sets;
                cand[r] = exchange_discards(g0, i, game_key(pseed, offset + (u64)g, (5ULL << 61) | ebase | ((u64)i << 6) | (u64)d));
            }
        }
    }
    __syncthreads();
    if (!plays) return;
    const u32 live = p.ncand * round_worlds;
    for (u32 s = lane; s < live; s += L) {
        const u32 r = s / round_worlds, lw = s - r * round_worlds, i = r / sets, d = r - i * sets;
        const int64_t u = g * 6 + (int64_t)i;
        const u32 o = on[u];
        if (!((o >> d) & 1u)) continue;
        const u32 it = net_list_slot(base[u], (u32)__popc(o & ((1u << d) - 1u)), round_worlds, lw);
        if (it >= bound) continue;
        Game h;
        unpack(h, a.x, a.y, b.x, b.y);
        world.load(t.slot0 + lw, h);
        const u32 dpk = cand[r];
        apply_exchange(h, i, dpk & 255, (dpk >> 8) & 255, (dpk >> 16) & 255);
        u64 x0, x1, y0, y1;
        pack(h, x0, x1, y0, y1);
        i01[it] = make_ulonglong2(x0, x1);
        i23[it] = make_ulonglong2(y0, y1);
        ikey[it] = game_key(pseed, offset + (u64)g, (3ULL << 62) | ebase | (63ULL << 22) | ((u64)(8u * i + d) << 16) | ((u64)(e0 + lw) << 10));
        ires[it] = VIEWER ? TK_PN_LIVE | (u64)p.declarer : TK_PN_LIVE;
    }
}

#define TK_EXCHANGE_NET_LIST_DEAL(NAME, VIEWER)                                                                                       \
    TK_KERNEL(TK_BLOCK, 128) void NAME(int64_t n, u32 bound, u64 pseed /* seed ^ salt */, u64 offset, u32 e0, u32 round_worlds,       \
                                      u32 sets, u32 lg, u32 seats, const uint8_t *__restrict__ seat_sets,                             \
                                      const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,                         \
                                      const Counters *__restrict__ cnt, const u32 *__restrict__ on, const u32 *__restrict__ base,     \
                                      ulonglong2 *__restrict__ i01, ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey,             \
                                      u64 *__restrict__ ires) {                                                                       \
        TK_VGPR_TOP(128, 127);                                                                                                        \
        playout_exchange_net_list_deal_body<VIEWER>(n, bound, pseed, offset, e0, round_worlds, sets, lg, seats, seat_sets, s01,       \
                                                    s23, cnt, on, base, i01, i23, ikey, ires);                                        \
    }
TK_EXCHANGE_NET_LIST_DEAL(k_playout_exchange_net_list_deal, false)
TK_EXCHANGE_NET_LIST_DEAL(k_playout_exchange_net_list_deal_value, true)
#undef TK_EXCHANGE_NET_LIST_DEAL

// Exchange, the sums and the choice: k_playout_exchange_net_sum reading compact slots; a row whose bit is off sums zeros.
TK_KERNEL(TK_BLOCK, 64) void k_playout_exchange_net_list_sum(int64_t n, u32 bound, u64 pseed /* seed ^ salt */, u64 offset, u32 worlds,
                                                            u32 sets, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                            const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                                            const Counters *__restrict__ cnt, const u64 *__restrict__ gkey,
                                                            const u32 *__restrict__ on, const u32 *__restrict__ base,
                                                            const u64 *__restrict__ ires, int4 *__restrict__ sum_out,
                                                            int8_t *__restrict__ choice_out, uint8_t *__restrict__ discards_out) {
    TK_VGPR_TOP(64, 63);
    __shared__ __attribute__((aligned(16))) int sums[(TK_BLOCK >> 4) * TK_PX_ROWS * 4];
    const PlayoutTeam t(4);
    const int64_t g = t.g;
    int *row = sums + t.team * (TK_PX_ROWS * 4);
    const u32 nrows = 6u * sets;
    if (g < n) {
        for (u32 r = t.lane; r < nrows; r += t.L) {
            const u32 i = r / sets, d = r - i * sets, o = on[g * 6 + i];
            int4 s = make_int4(0, 0, 0, 0);
            if ((o >> d) & 1u) {
                const u32 first = net_list_slot(base[g * 6 + i], (u32)__popc(o & ((1u << d) - 1u)), worlds, 0u);
                for (u32 w = 0; w < worlds; w++) {
                    const u64 sc = first + w < bound ? ires[first + w] : 0ULL;
                    s.x += (int)(int16_t)sc; s.y += (int)(int16_t)(sc >> 16); s.z += (int)(int16_t)(sc >> 32); s.w += (int)(int16_t)(sc >> 48);
                }
            }
            reinterpret_cast<int4 *>(row)[r] = s;
        }
    }
    __syncthreads();
    if (g >= n) return;
    if (sum_out)
        for (u32 r = t.lane; r < nrows; r += t.L) sum_out[g * nrows + r] = reinterpret_cast<const int4 *>(row)[r];
    if ((choice_out || discards_out) && t.lane == 0) {
        Game g0;
        load_game(g0, s01, s23, g);
        const ExchangePosition p = exchange_position(g0, seat_sets, seats, sets, g);
        int ch = -1;
        u32 dpk = 0xFFFFFFu;
        if (p.takes_part) {                              // the first candidate at the maximum of the declarer's sums
            const u32 best = best_row(row, p.ncand, p.declarer), i = best / sets, d = best - i * sets;
            ch = (int)i;
            dpk = exchange_discards(g0, i, game_key(pseed, offset + (u64)g, (5ULL << 61) | ((u64)cnt[g].episode << 28) | ((u64)i << 6) | (u64)d));
        } else if (p.waiting) {                          // the Bot's own exchange: group 0, its sampler under the game's key
            ch = 0;
            dpk = exchange_discards(g0, 0u, gkey[g]);
        }
        if (choice_out) choice_out[g] = (int8_t)ch;
        if (discards_out) {
            discards_out[g * 3 + 0] = (uint8_t)dpk; discards_out[g * 3 + 1] = (uint8_t)(dpk >> 8);
            discards_out[g * 3 + 2] = (uint8_t)(dpk >> 16);
        }
    }
}

// Bids, second launch (after k_bid_deal): one thread a unit.
TK_KERNEL(TK_BLOCK, 64) void k_playout_bids_net_list_init(int64_t n, u32 contracts, u32 pass_value, u32 seats,
                                                         const uint8_t *__restrict__ seat_sets, const u64 *__restrict__ deal,
                                                         u32 *__restrict__ on) {
    TK_VGPR_TOP(64, 63);
    const int64_t u = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (u >= n * 4) return;
    const int64_t g = u >> 2;
    u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
    if ((deal[g] | deal[n + g] | deal[2 * n + g] | deal[3 * n + g]) == 0) set = 0;      // an invalid deal row
    on[u] = bid_list_on(contracts, pass_value, (set >> ((u32)u & 3u)) & 1u);
}

// Bids, the items, for the list launch and for every halving round (§8.23): k_playout_bids_net_deal's team, keys and item setup
// (VIEWER: _deal_value's marker, PASS: _deal_value_pass's pass item) over the unit's live rows, in the worlds e0 + lw, lw <
// round_worlds, dealt into the team's world slots 0 .. round_worlds - 1; the two barriers per viewer stand outside every test
// of the unit's word.  The list launch is e0 = 0, round_worlds = worlds, on the init kernel's words: a viewer takes part — its
// seat bit with a valid deal row — exactly where its on word is non-zero, since bid_list_on is `part ? rows : 0` and rows is
// never 0 for contracts >= 1.
template <bool VIEWER, bool PASS>
__device__ __forceinline__ void playout_bids_net_list_deal_body(int64_t n, u32 bound, u64 pseed, u64 offset, u32 episode, u32 e0,
                                                                u32 round_worlds, u32 lg, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                                const u64 *__restrict__ deal, const u32 *__restrict__ on,
                                                                const u32 *__restrict__ base, ulonglong2 *__restrict__ i01,
                                                                ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey,
                                                                u64 *__restrict__ ires) {
    static_assert(VIEWER || !PASS, "the pass item carries its viewer");
    __shared__ u64 world_a[TK_PO_WORLD_SLOTS], world_b[TK_PO_WORLD_SLOTS], world_ids[TK_PO_WORLD_SLOTS];
    const PlayoutTeam t(lg, round_worlds);
    const u32 L = t.L, lane = t.lane, slot0 = t.slot0;
    const int64_t g = t.g;
    u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, tal = 0;
    if (g < n) { h0 = deal[g]; h1 = deal[n + g]; h2 = deal[2 * n + g]; h3 = deal[3 * n + g]; tal = deal[4 * n + g]; }
    const u64 ebase = (u64)episode << 28;
#pragma unroll 1
    for (u32 v = 0; v < 4; v++) {
        const u32 o = g < n ? on[g * 4 + v] : 0u;        // (on: only viewers of the seat set with a valid deal row)
        __syncthreads();                                 // the last viewer's items have read their worlds
        if (o) {
            for (u32 lw = lane; lw < round_worlds; lw += L) {
                u64 A, B, ids;
                bid_world(h0, h1, h2, h3, tal, v, game_key(pseed, offset + (u64)g, (2ULL << 61) | ebase | ((u64)v << 6) | (u64)(e0 + lw)), A, B, ids);
                world_a[slot0 + lw] = A; world_b[slot0 + lw] = B; world_ids[slot0 + lw] = ids;
            }
        }
        __syncthreads();
        if (o) {
            const u32 first = base[g * 4 + v];           // (bit 19 only under the PASS form: the launcher pairs them)
            const u32 count = net_list_count(o, round_worlds);
            for (u32 s = lane; s < count; s += L) {
                const u32 q = s / round_worlds, lw = s - q * round_worlds, w = e0 + lw, r = kth_bit_word(o, 0u, q);
                const u32 it = net_list_slot(first, q, round_worlds, lw);
                if (it >= bound) continue;
                const u64 pkey = game_key(pseed, offset + (u64)g, (3ULL << 61) | ebase | ((u64)v << 26) | ((u64)r << 21) | ((u64)w << 15));
                Game h;
                if constexpr (PASS) {                    // (k_playout_bids_pass's one setup for both kinds of item)
                    u32 ct = bid_row_contract(r), d = ct == TK_KLOP ? 0u : v, kg = bid_row_king(r);
                    if (r == (u32)TK_BID_PASS_ROW) pass_round(pkey, v, ct, d, kg);
                    bid_game_as(h, world_a[slot0 + lw], world_b[slot0 + lw], world_ids[slot0 + lw], ct, d, kg);
                } else {
                    bid_game(h, world_a[slot0 + lw], world_b[slot0 + lw], world_ids[slot0 + lw], r, v);
                }
                if (h.phase == TK_PHASE_EXCHANGE) bot_exchange(h, pkey);
                u64 x0, x1, y0, y1;
                pack(h, x0, x1, y0, y1);
                i01[it] = make_ulonglong2(x0, x1);
                i23[it] = make_ulonglong2(y0, y1);
                ikey[it] = pkey;
                ires[it] = VIEWER ? TK_PN_LIVE | (u64)v : TK_PN_LIVE;
            }
        }
    }
}

#define TK_BIDS_NET_LIST_DEAL(NAME, VIEWER, PASS)                                                                                     \
    TK_KERNEL(TK_BLOCK, 128) void NAME(int64_t n, u32 bound, u64 pseed /* seed ^ salt */, u64 offset, u32 episode, u32 e0,            \
                                      u32 round_worlds, u32 lg, u32 seats, const uint8_t *__restrict__ seat_sets,                     \
                                      const u64 *__restrict__ deal, const u32 *__restrict__ on, const u32 *__restrict__ base,         \
                                      ulonglong2 *__restrict__ i01, ulonglong2 *__restrict__ i23, u64 *__restrict__ ikey,             \
                                      u64 *__restrict__ ires) {                                                                       \
        TK_VGPR_TOP(128, 127);                                                                                                        \
        playout_bids_net_list_deal_body<VIEWER, PASS>(n, bound, pseed, offset, episode, e0, round_worlds, lg, seats, seat_sets,       \
                                                      deal, on, base, i01, i23, ikey, ires);                                          \
    }
TK_BIDS_NET_LIST_DEAL(k_playout_bids_net_list_deal, false, false)
TK_BIDS_NET_LIST_DEAL(k_playout_bids_net_list_deal_value, true, false)
TK_BIDS_NET_LIST_DEAL(k_playout_bids_net_list_deal_value_pass, true, true)
#undef TK_BIDS_NET_LIST_DEAL

// Bids, the sums: one thread per (game, viewer, row); the VIEWER's 16 bits of the row's items, found through the unit's
// word, summed over the worlds in integers.  A row whose bit is off gets 0: every row is written.
TK_KERNEL(TK_BLOCK, 64) void k_playout_bids_net_list_sum(int64_t rows /* n * 4 * TAROK_BID_ROWS */, u32 bound, u32 worlds,
                                                        const u32 *__restrict__ on, const u32 *__restrict__ base,
                                                        const u64 *__restrict__ ires, int *__restrict__ sum_out) {
    TK_VGPR_TOP(64, 63);
    const int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= rows) return;
    const int64_t u = i / TAROK_BID_ROWS;
    const u32 r = (u32)(i - u * TAROK_BID_ROWS), v = (u32)(u & 3), o = on[u];
    int s = 0;
    if ((o >> r) & 1u) {
        const u32 first = net_list_slot(base[u], (u32)__popc(o & ((1u << r) - 1u)), worlds, 0u);
        for (u32 w = 0; w < worlds; w++) {
            const u64 sc = first + w < bound ? ires[first + w] : 0ULL;
            s += (int)(int16_t)(sc >> (16 * v));
        }
    }
    sum_out[i] = s;
}

// ---------------------------------------------------------------------------
// tarok_playout_exchange_net_halving / tarok_playout_bids_net_halving: sequential halving over the lists above.
// Beside its `on` word a unit keeps an `alive` word (the arms still in the race; on = alive, plus the pass bit for the bids,
// while the game or unit plays rounds, else 0), and every row a running sum and a count in the scratch.  A round is
// tarok_playout_cards_net_halving's: the scan over the on words, the round's items in its worlds e0 .. e1 - 1 alone, under
// their true indices, the playouts on the round's total, the sums and the survivor rule (front_halving_stays, one arm a lane).
// The round's items are §8.22's deal kernels at the round's e0, round_worlds and bound; this section adds the init and the sums.

// Exchange, first launch: one thread a unit: the on and alive words, the unit's running sums and counts zeroed.
TK_KERNEL(TK_BLOCK, 64) void k_playout_exchange_net_halving_init(int64_t units, u32 sets, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                                const ulonglong2 *__restrict__ s01, const ulonglong2 *__restrict__ s23,
                                                                u32 *__restrict__ on, u32 *__restrict__ alive, int4 *__restrict__ rsum,
                                                                int *__restrict__ rcnt) {
    TK_VGPR_TOP(64, 63);
    const int64_t u = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (u >= units) return;
    const int64_t g = u / 6;
    Game g0;
    load_game(g0, s01, s23, g);
    const ExchangePosition p = exchange_position(g0, seat_sets, seats, sets, g);
    const u32 o = exchange_list_on(g0.contract, (u32)(u - g * 6), sets, p.takes_part);
    on[u] = o;
    alive[u] = o;
    for (u32 d = 0; d < sets; d++) {
        rsum[u * sets + d] = make_int4(0, 0, 0, 0);
        rcnt[u * sets + d] = 0;
    }
}

// Exchange, a round's sums and the survivor rule: 16 lanes a game.  A lane takes the rows r = lane, lane + 16, lane + 32: a row
// that played the round adds its round_worlds results, in integers, to its running sums and sets its count to the round's end
// e1; the declarer's column of every row goes to the team's [48] ints in LDS.  After the barrier, not the last round: each
// alive row's lane counts the arms that beat it (front_halving_stays) and ORs its bit into the team's six next words; after a
// second barrier lanes 0..5 write the units' alive and on words — on = 0 once one arm is left.  The last round: every row's
// sums and count are written, and the choice is the first row at the maximum of the declarer's sums among the rows alive.
TK_KERNEL(TK_BLOCK, 64) void k_playout_exchange_net_halving_sum(int64_t n, u32 bound, u64 pseed /* seed ^ salt */, u64 offset, u32 e1,
                                                               u32 round_worlds, u32 last, u32 sets, u32 seats,
                                                               const uint8_t *__restrict__ seat_sets, const ulonglong2 *__restrict__ s01,
                                                               const ulonglong2 *__restrict__ s23, const Counters *__restrict__ cnt,
                                                               const u64 *__restrict__ gkey, const u64 *__restrict__ ires,
                                                               u32 *__restrict__ on, u32 *__restrict__ alive, const u32 *__restrict__ base,
                                                               int4 *__restrict__ rsum, int *__restrict__ rcnt, int4 *__restrict__ sum_out,
                                                               int *__restrict__ count_out, int8_t *__restrict__ choice_out,
                                                               uint8_t *__restrict__ discards_out) {
    TK_VGPR_TOP(64, 63);
    __shared__ int vals[(TK_BLOCK >> 4) * TK_PX_ROWS];
    __shared__ u32 nexts[(TK_BLOCK >> 4) * 6];
    const PlayoutTeam t(4);
    const int64_t g = t.g;
    int *val = vals + t.team * TK_PX_ROWS;
    u32 *next = nexts + t.team * 6;
    const u32 nrows = 6u * sets;
    u64 al = 0;
    ExchangePosition p;
    Game g0;
    if (t.lane < 6u) next[t.lane] = 0u;
    if (g < n) {
        load_game(g0, s01, s23, g);
        p = exchange_position(g0, seat_sets, seats, sets, g);
        for (u32 i = 0; i < 6; i++) al |= (u64)alive[g * 6 + i] << (i * sets);
        for (u32 r = t.lane; r < nrows; r += t.L) {
            const u32 i = r / sets, d = r - i * sets, o = on[g * 6 + i];
            int4 s = rsum[g * nrows + r];
            int c = rcnt[g * nrows + r];
            if ((o >> d) & 1u) {
                const u32 first = net_list_slot(base[g * 6 + i], (u32)__popc(o & ((1u << d) - 1u)), round_worlds, 0u);
                for (u32 w = 0; w < round_worlds; w++) {
                    const u64 sc = first + w < bound ? ires[first + w] : 0ULL;
                    s.x += (int)(int16_t)sc; s.y += (int)(int16_t)(sc >> 16); s.z += (int)(int16_t)(sc >> 32); s.w += (int)(int16_t)(sc >> 48);
                }
                c = (int)e1;
                rsum[g * nrows + r] = s;
                rcnt[g * nrows + r] = c;
            }
            val[r] = p.declarer == 0 ? s.x : (p.declarer == 1 ? s.y : (p.declarer == 2 ? s.z : s.w));
            if (last) {
                if (sum_out) sum_out[g * nrows + r] = s;
                if (count_out) count_out[g * nrows + r] = c;
            }
        }
    }
    __syncthreads();
    if (!last) {
        if (g < n)
            for (u32 r = t.lane; r < nrows; r += t.L)
                if (((al >> r) & 1ULL) && front_halving_stays(val, 1u, al, r)) atomicOr(next + r / sets, 1u << (r % sets));
        __syncthreads();
        if (g < n && t.lane < 6u) {
            u32 left = 0;
            for (u32 i = 0; i < 6; i++) left += (u32)__popc(next[i]);
            alive[g * 6 + t.lane] = next[t.lane];
            on[g * 6 + t.lane] = left > 1u ? next[t.lane] : 0u;      // a game down to one candidate plays no further round
        }
        return;
    }
    if (g >= n || t.lane != 0u || (!choice_out && !discards_out)) return;
    int ch = -1;
    u32 dpk = 0xFFFFFFu;
    if (p.takes_part) {                                  // the first alive candidate at the maximum of the declarer's sums
        u32 best = 0;
        int top = 0;
        bool none = true;
#pragma nounroll
        for (u64 rest = al; rest; rest &= rest - 1ULL) {
            const u32 r = (u32)__builtin_ctzll(rest);
            const int v = val[r];
            if (none || v > top) { top = v; best = r; none = false; }
        }
        const u32 i = best / sets, d = best - i * sets;
        ch = (int)i;
        dpk = exchange_discards(g0, i, game_key(pseed, offset + (u64)g, (5ULL << 61) | ((u64)cnt[g].episode << 28) | ((u64)i << 6) | (u64)d));
    } else if (p.waiting) {                              // the Bot's own exchange: group 0, its sampler under the game's key
        ch = 0;
        dpk = exchange_discards(g0, 0u, gkey[g]);
    }
    if (choice_out) choice_out[g] = (int8_t)ch;
    if (discards_out) {
        discards_out[g * 3 + 0] = (uint8_t)dpk; discards_out[g * 3 + 1] = (uint8_t)(dpk >> 8);
        discards_out[g * 3 + 2] = (uint8_t)(dpk >> 16);
    }
}

// Bids, second launch (after k_bid_deal): one thread a unit: the on word (the rows, and row 19 with pass_value), the alive word
// (the rows alone: the pass is the bar, not an arm), the unit's running sums and counts zeroed.
TK_KERNEL(TK_BLOCK, 64) void k_playout_bids_net_halving_init(int64_t n, u32 contracts, u32 pass_value, u32 seats,
                                                            const uint8_t *__restrict__ seat_sets, const u64 *__restrict__ deal,
                                                            u32 *__restrict__ on, u32 *__restrict__ alive, int4 *__restrict__ rsum,
                                                            int4 *__restrict__ rcnt) {
    TK_VGPR_TOP(64, 63);
    const int64_t u = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (u >= n * 4) return;
    const int64_t g = u >> 2;
    u32 set = seat_sets ? (u32)seat_sets[g] & 15u : seats;
    if ((deal[g] | deal[n + g] | deal[2 * n + g] | deal[3 * n + g]) == 0) set = 0;      // an invalid deal row
    const u32 o = bid_list_on(contracts, pass_value, (set >> ((u32)u & 3u)) & 1u);
    on[u] = o;
    alive[u] = o & ~(1u << TK_BID_PASS_ROW);
    for (u32 q = 0; q < TAROK_BID_ROWS / 4; q++) {
        rsum[u * (TAROK_BID_ROWS / 4) + q] = make_int4(0, 0, 0, 0);
        rcnt[u * (TAROK_BID_ROWS / 4) + q] = make_int4(0, 0, 0, 0);
    }
}

// Bids, a round's sums and the survivor rule: 32 lanes a unit, lane r < 20 its row r.  A row that played the round adds the
// VIEWER's 16 bits of its round_worlds results to its running sum and sets its count to e1; the sums go to the team's [20]
// ints in LDS.  After the barrier, not the last round: an alive row's lane counts the arms that beat it and ORs its bit into
// the team's next word; after a second barrier lane 0 writes the unit's alive word and its on word — the survivors and the
// pass bit the unit had, or 0 once one arm is left.  The last round: every row's sum, count and value are written.
TK_KERNEL(TK_BLOCK, 64) void k_playout_bids_net_halving_sum(int64_t units, u32 bound, u32 e1, u32 round_worlds, u32 last, u32 worlds,
                                                           const u64 *__restrict__ ires, u32 *__restrict__ on, u32 *__restrict__ alive,
                                                           const u32 *__restrict__ base, int *__restrict__ rsum, int *__restrict__ rcnt,
                                                           int *__restrict__ sum_out, int *__restrict__ count_out,
                                                           int *__restrict__ value_out) {
    TK_VGPR_TOP(64, 63);
    __shared__ int vals[(TK_BLOCK >> 5) * 32];
    __shared__ u32 nexts[TK_BLOCK >> 5];
    const PlayoutTeam t(5);
    const int64_t u = t.g;
    const u32 r = t.lane, v = (u32)(u & 3);
    int *val = vals + t.team * 32;
    u32 o = 0, al = 0;
    if (r == 0u) nexts[t.team] = 0u;
    if (u < units) {
        o = on[u]; al = alive[u];
        if (r < (u32)TAROK_BID_ROWS) {
            int s = rsum[u * TAROK_BID_ROWS + r], c = rcnt[u * TAROK_BID_ROWS + r];
            if ((o >> r) & 1u) {
                const u32 first = net_list_slot(base[u], (u32)__popc(o & ((1u << r) - 1u)), round_worlds, 0u);
                for (u32 w = 0; w < round_worlds; w++) {
                    const u64 sc = first + w < bound ? ires[first + w] : 0ULL;
                    s += (int)(int16_t)(sc >> (16 * v));
                }
                c = (int)e1;
                rsum[u * TAROK_BID_ROWS + r] = s;
                rcnt[u * TAROK_BID_ROWS + r] = c;
            }
            val[r] = s;
            if (last) {
                if (sum_out) sum_out[u * TAROK_BID_ROWS + r] = s;
                if (count_out) count_out[u * TAROK_BID_ROWS + r] = c;
                if (value_out) value_out[u * TAROK_BID_ROWS + r] = front_halving_value(s, (int)worlds, c);
            }
        }
    }
    if (last) return;                                    // (launch-uniform)
    __syncthreads();
    if (u < units && ((al >> r) & 1u) && front_halving_stays(val, 1u, (u64)al, r)) atomicOr(nexts + t.team, 1u << r);
    __syncthreads();
    if (u < units && r == 0u) {
        const u32 next = nexts[t.team];
        alive[u] = next;
        on[u] = (next & (next - 1u)) != 0u ? next | (o & (1u << TK_BID_PASS_ROW)) : 0u;     // one arm left: no further round
    }
}

// ---------------------------------------------------------------------------
// The reference agent's transition targets in its own form: what Nevronski_igralec.rezultat_stiha
// builds per trick and rezultat_igre completes (Igralec.py:387-446), for every (trick, game, seat) of a recorded
// rollout of whole tricks:  dy[54] = -70 on the cards that were not legal at the seat's decision (:392-393), on the
// card it played +Roka.vrednost_stiha(trick) if it took the trick, else minus that (:412-416: every contract runs
// this branch, the Klop / Berac branches of :394-409 compare a dict with a string), plus final_reword_factor times
// next_max (:441), where next_max is the agent's own estimate at its next decision (:351,417-418; `next_q`, the
// caller's: NULL = 0) or, on the game's last trick, the final reward (:439, the rewards of TAROK_REWARD_REF).
// Rows [T,N] as the step kernels wrote them; T a multiple of 4 and the rollout starts on a trick boundary (games are
// whole tricks long, so every slot stays trick-aligned through the auto-resets): trick b = rows 4b .. 4b+3.
// Parity unpinned for this assembly (the reference holds no fixture and Igralec.py cannot be imported); its inputs —
// legal masks, cards, trick values and winners, final scores — are pinned by the reference's recorded runs.
// Workgroup = 64 slots x 4 seats: one thread per (slot, seat) builds its row's description, then the 256 threads
// write the 64 x 4 x 54 floats of the workgroup as full lines.
#define TG_SLOTS 64
TK_KERNEL(256, 64) void k_targets_ref(int64_t n, int T, const u64 *__restrict__ obs_before, const uint8_t *__restrict__ action,
                                                    const uint16_t *__restrict__ trick, const uint8_t *__restrict__ done,
                                                    const int16_t *__restrict__ reward, const float *__restrict__ next_q, float factor,
                                                    float4 *__restrict__ dy, uint8_t *__restrict__ meta) {
    TK_VGPR_TOP(64, 63);
    __shared__ uint2 mask_s[256];
    __shared__ float val_s[256];
    __shared__ u32 card_s[256];
    const u32 tid = threadIdx.x, b = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * TG_SLOTS, i = i0 + (tid >> 2);
    const u32 s = tid & 3;
    u64 legal = TK_DECK;                                      // (rows without a decision: all zeros)
    u32 card = 255, flags = 0;
    float val = 0.f;
    if (i < n) {
        int found = -1;
        for (int k = 0; k < 4; k++) {
            u64 ob = obs_before[(int64_t)(4 * b + k) * n + i];
            bool mine = ((u32)(ob >> TAROK_OBS_SEAT_SHIFT) & 3u) == s && action[(int64_t)(4 * b + k) * n + i] < 54 && found < 0;
            if (mine) { found = k; legal = ob & TAROK_OBS_MASK; card = action[(int64_t)(4 * b + k) * n + i]; }
        }
        int64_t last = (int64_t)(4 * b + 3) * n + i;
        u32 tw = trick[last];
        if (found >= 0 && (tw & 0x8000u)) {
            flags = 1;
            float tv = (float)((tw >> 4) & 0x7FFu);
            val = ((tw & 3u) == s) ? tv : -tv;                // sem_pobral (Klop.py:76-77, Navadna_igra.py:138-139)
            float next_max = 0.f;
            if (done[last]) { next_max = (float)reward[last * 4 + s]; flags |= 2; }
            else if ((int)(4 * b + 7) < T) {
                int nk = -1;
                for (int k = 0; k < 4; k++) {
                    u64 ob = obs_before[(int64_t)(4 * b + 4 + k) * n + i];
                    if (((u32)(ob >> TAROK_OBS_SEAT_SHIFT) & 3u) == s && nk < 0) nk = k;
                }
                if (nk >= 0) next_max = next_q ? next_q[(int64_t)(4 * b + 4 + nk) * n + i] : 0.f;
                else flags |= 4;
            } else flags |= 4;                                // the seat's next decision lies beyond the rollout
            val += factor * next_max;
        } else { legal = TK_DECK; card = 255; }
        meta[((int64_t)b * n + i) * 4 + s] = (uint8_t)flags;
    }
    mask_s[tid] = make_uint2(TK_LO(legal), TK_HI(legal));
    val_s[tid] = val;
    card_s[tid] = card;
    __syncthreads();
    int64_t slots = n - i0 < TG_SLOTS ? n - i0 : TG_SLOTS;
    u32 quads = (u32)(slots * 4 * 54 / 4);                    // float4 pieces of this workgroup's rows
    float4 *out = dy + ((int64_t)b * n + i0) * 54;            // (row (b, i, seat) starts at float ((b n + i) 4 + seat) 54)
    for (u32 e4 = tid; e4 < quads; e4 += 256) {
        float v[4];
#pragma unroll
        for (u32 k = 0; k < 4; k++) {
            u32 e = 4 * e4 + k, row = e / 54, c = e - 54 * row;
            uint2 m = mask_s[row];
            u32 bit = c < 32 ? (m.x >> c) & 1u : (m.y >> (c - 32)) & 1u;
            v[k] = c == card_s[row] ? val_s[row] : (bit ? 0.f : -70.f);
        }
        out[e4] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

#include "tarok_learner.inc"

TK_KERNEL(TK_BLOCK, 64) void k_counters(int64_t n, const Counters *__restrict__ cnt, u32 *__restrict__ ep,
                                                      int4 *__restrict__ score_sum) {
    TK_VGPR_TOP(64, 63);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (ep) ep[i] = cnt[i].episode;
    if (score_sum) score_sum[i] = cnt[i].score_sum;
}

// canonical lanes for parity checks: H0-3, P0-3, TAL, META (tarok_env.h); store(lane, value) takes the ten of one game
template <class Store>
__device__ __forceinline__ void state_lanes(const Game &g, Store store) {
    u64 on_table = 0;
    for (u32 j = 0; j < g.nt; j++) on_table |= 1ULL << ((g.trick >> (6 * j)) & 63);
    u64 won = g.C & ~talon_unowned(g) & ~on_table;
    for (u32 s = 0; s < 4; s++) {
        store((int)s, hand_of(g, s));
        store((int)(4 + s), seat_cards(g, s) & won);
    }
    store(8, g.talon);
    u64 m = g.trick;
    m |= (u64)g.nt << 24;
    m |= (u64)g.leader << 27;
    m |= (u64)g.trick_no << 29;
    m |= (u64)g.contract << 33;
    m |= (u64)g.declarer << 37;
    m |= (u64)(has_king(g.contract) ? g.king : 7) << 39;
    m |= (u64)g.team << 42;
    m |= (u64)(g.contract == TK_KLOP ? g.tl : 0) << 46;
    m |= (u64)(has_exchange(g.contract) ? g.tl : 7) << 49;
    m |= (u64)g.phase << 52;
    m |= (u64)g.error << 54;
    store(9, m);
}

TK_KERNEL(TK_BLOCK, 64) void k_get_state(int64_t n, const ulonglong2 *__restrict__ s01,
                                                       const ulonglong2 *__restrict__ s23, u64 *__restrict__ out) {
    TK_VGPR_TOP(64, 63);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    Game g;
    load_game(g, s01, s23, i);
    state_lanes(g, [&](int lane, u64 v) { out[(int64_t)lane * n + i] = v; });
}

// inverse of k_get_state: rebuild the packed pairs from canonical lanes (checkpoint restore,
// hand-built positions).  Cards on the table go back to whoever played them, the un-owned
// talon to where setup_game parks it.
TK_KERNEL(TK_BLOCK, 64) void k_set_state(int64_t n, const u64 *__restrict__ in,
                                                       ulonglong2 *__restrict__ s01, ulonglong2 *__restrict__ s23,
                                                       const Counters *__restrict__ cnt) {
    TK_VGPR_TOP(64, 63);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 m = in[9 * n + i];
    Game g;
    g.trick = (u32)m & 0xFFFFFF;
    g.nt = (u32)(m >> 24) & 7; g.leader = (u32)(m >> 27) & 3; g.trick_no = (u32)(m >> 29) & 15;
    g.contract = (u32)(m >> 33) & 15; g.declarer = (u32)(m >> 37) & 3;
    u32 king = (u32)(m >> 39) & 7;
    g.king = king == 7 ? 0 : king;
    g.team = (u32)(m >> 42) & 15;
    u32 talon_left = (u32)(m >> 46) & 7, choice = (u32)(m >> 49) & 7;
    g.phase = (u32)(m >> 52) & 3; g.error = (u32)(m >> 54) & 1;
    g.epar = TK_LINE(cnt[i].episode);
    {   // lines on a refill list stay off limits for the next launch
        ulonglong2 old = s23[i];
        g.cprev = ((u32)(old.y >> 62) & 3u) | (((u32)(old.x >> 62) & 3u) << 2);
    }
    g.talon = in[8 * n + i] & ((1ULL << 36) - 1);
    g.tl = g.contract == TK_KLOP ? talon_left : ((has_exchange(g.contract) || g.contract == TK_SOLO_BREZ) ? choice : 0);
    u64 seatc[4];
    u64 piles = 0;
    for (u32 s = 0; s < 4; s++) {
        u64 h = in[(int64_t)s * n + i] & TK_DECK, p = in[(int64_t)(4 + s) * n + i] & TK_DECK;
        seatc[s] = h | p;
        piles |= p;
    }
    u64 on_table = 0;
    for (u32 j = 0; j < g.nt && j < 4; j++) {
        u64 b = 1ULL << ((g.trick >> (6 * j)) & 63);
        on_table |= b;
        seatc[(g.leader + j) & 3] |= b;
    }
    u64 unowned = talon_unowned(g);                 // depends only on contract / tl / talon ids
    u32 o = g.contract == TK_KLOP ? 0u : (u32)__builtin_ctz(~g.team & 15u);
    seatc[o & 3] |= unowned;
    g.A = seatc[1] | seatc[3];
    g.B = seatc[2] | seatc[3];
    g.C = piles | on_table | unowned;
    store_game(g, s01, s23, i);
}

#include "tarok_front.inc"


// ---------------------------------------------------------------------------
// tarok_debug_refill_selftest: the refill role AS EACH STEP KERNEL COMPILES IT, fed with lists built by hand — every slot of
// every group, `per_slot` episodes each, on both parities — and every line it writes compared with a straight re-deal by a
// kernel of its own.  Round 3's corruption was a dealt-ahead game WRITTEN wrong by the refill loop of one build (a gfx950
// erratum, see TK_VGPR_TOP); no test looked at the lines themselves, and only lists of several hundred entries — four
// passes of the loop on full waves — showed it.  This is that test (tests/test_gpu_parity.py), for any build.
__global__ __launch_bounds__(TK_BLOCK) TK_VGPR_BUDGET(64) void k_dbg_fill_lists(u64 *rlist, u32 *rcount, int64_t n, u32 per_slot, u32 ep0, u32 order) {
    TK_VGPR_TOP(64, 63);
    u32 g = blockIdx.x;
    // the slots the group has: a partial last group lists only those (the refill role deals what it is told to, and a
    // line of a slot >= n lies behind the end of the lines' allocation)
    const u32 have = (u32)min((int64_t)TK_BLOCK, n - (int64_t)g * TK_BLOCK);
    if (order == 2 && have % 37u == 0) order = 1;                // (t * 37 + 11 mod `have` must stay a permutation)
    for (u32 idx = threadIdx.x; idx < per_slot * have; idx += TK_BLOCK) {
        u32 k = idx / have, t = idx % have;
        if (order == 1) t = have - 1 - t;
        if (order == 2) t = (t * 37u + 11u) % have;
        u64 en = ((u64)(ep0 + 1 + k) << 32) | t;
        rlist[((int64_t)g * 2 + 0) * TK_REFILL_CAP + idx] = en;
        rlist[((int64_t)g * 2 + 1) * TK_REFILL_CAP + idx] = en;
    }
    if (threadIdx.x == 0) {
        rcount[TK_RC(g, 0)] = per_slot * have; rcount[TK_RC(g, 1)] = per_slot * have;
        rcount[TK_RC(g, 2)] = 0; rcount[TK_RC(g, 3)] = 0;
    }
}
__global__ __launch_bounds__(TK_BLOCK) TK_VGPR_BUDGET(64) void k_dbg_clear_lines(Aux *aux, int64_t n) {
    TK_VGPR_TOP(64, 63);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    for (int b = 0; b < TK_AHEAD; b++) {
        AuxLine *ln = &aux[i].line[b];
        ln->n01 = make_ulonglong2(0, 0); ln->n23 = make_ulonglong2(0, 0); ln->nkey = 0; ln->nep = 0xFFFFFFFFu;
    }
}
// out[0] = lines that differ; out[1 + 6 r ..] = {slot, episode, x0 read, x0 expected, y0 read, y0 expected} of the first eight
__global__ __launch_bounds__(TK_BLOCK) TK_VGPR_BUDGET(128) void k_dbg_check_lines(Aux *aux, int64_t n, u64 seed, u64 offset, int mix, u32 per_slot,
                                                                                  u32 ep0, unsigned long long *out) {
    TK_VGPR_TOP(128, 127);
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (i >= n) return;
    for (u32 k = 0; k < per_slot; k++) {
        u32 episode = ep0 + 1 + k;
        u64 key = game_key(seed, offset + (u64)i, (u64)episode);
        u64 h0, h1, h2, h3, tal;
        deal_thread(key, h0, h1, h2, h3, tal);
        u32 c, d, kk;
        sample_setup(key, mix, c, d, kk);
        Game g;
        setup_game(g, h0, h1, h2, h3, tal, c, d, kk);
        g.epar = TK_LINE(episode); g.cprev = 0;
        if (g.phase == TK_PHASE_EXCHANGE) bot_exchange(g, key);
        ulonglong2 ea, eb;
        pack(g, ea.x, ea.y, eb.x, eb.y);
        const AuxLine *ln = &aux[i].line[TK_LINE(episode)];
        ulonglong2 na = ln->n01, nb = ln->n23;
        if (ea.x != na.x || ea.y != na.y || eb.x != nb.x || eb.y != nb.y || key != ln->nkey || ln->nep != episode) {
            unsigned long long r = atomicAdd(&out[0], 1ULL);
            if (r < 8) {
                unsigned long long *o = out + 1 + 6 * r;
                o[0] = (u64)i; o[1] = episode; o[2] = na.x; o[3] = ea.x; o[4] = nb.x; o[5] = eb.x;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

const char *tarok_strerror(int code) {
    switch (code) {
        case TAROK_OK: return "ok";
        case TAROK_EINVAL: return "invalid argument";
        case TAROK_EHIP: return "HIP runtime error (see tarok_last_hip_error)";
        case TAROK_ENOMEM: return "out of device memory";
        case TAROK_ENODEV: return "no usable GPU";
        default: return "unknown error";
    }
}

int tarok_abi_version(void) { return TAROK_ABI_VERSION; }
int tarok_last_hip_error(void) { return g_last_hip; }

int tarok_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int tarok_create(tarok_env **out, int device, int64_t n_games, uint64_t game_offset, uint64_t seed, int mix, int flags) {
    if (!out || n_games <= 0 || n_games > (1LL << 31) || (flags & ~TAROK_HISTORY)) return TAROK_EINVAL;
    if (!(mix == TAROK_MIX_ALL || mix == TAROK_MIX_NAVADNA3 || mix == TAROK_MIX_BOT || (mix >= TAROK_MIX_FIXED && mix < TAROK_MIX_FIXED + 10))) return TAROK_EINVAL;
    if (device < 0 || device >= tarok_device_count()) return TAROK_ENODEV;
    HIPCHK(hipSetDevice(device));
    tarok_env *e = new tarok_env();
    memset(e, 0, sizeof *e);
    e->device = device; e->n = n_games; e->offset = game_offset; e->seed = seed; e->mix = mix; e->flags = flags;
    // latency-bound batches keep refill workgroups single-pass; throughput-bound ones pack them dense
    e->refill_fan = n_games >= (1 << 20) ? TK_REFILL_FAN : (n_games >= (1 << 18) ? 4 : 1);
    // Bulk deals where a launch is a handful of workgroups per CU and its refill workgroups' deals are its tail (65,536
    // games: -8 % per lock-step, 262,144: -7 %); where the batch streams the deals' instructions add to the launch
    // wherever they run, and a whole stretch of launches' worth at once cost what they cost one trick at a time (profiles/r03_ab_step.txt (e))
    e->lazy_refill = n_games < (1 << 20) ? 1 : 0;
    e->temperature = 1.f; e->inv_t = 1.f;      // play mode (1, 0): epsilon, thr, greedy and mode_on are 0
    size_t stale_bytes = (size_t)((n_games + TK_PF_SLOTS - 1) / TK_PF_SLOTS) * TK_PF_SLOTS * sizeof(uint16_t);
    hipError_t r = hipMalloc((void **)&e->s01, (size_t)n_games * sizeof(ulonglong2));
    if (r == hipSuccess) r = hipMalloc((void **)&e->s23, (size_t)n_games * sizeof(ulonglong2));
    if (r == hipSuccess) r = hipMalloc((void **)&e->aux, (size_t)n_games * sizeof(Aux));
    if (r == hipSuccess) r = hipMalloc((void **)&e->cnt, (size_t)n_games * sizeof(Counters));
    if (r == hipSuccess) r = hipMalloc((void **)&e->nstale, stale_bytes);
    if (r == hipSuccess) r = hipMalloc((void **)&e->gkey, (size_t)n_games * sizeof(u64));
    if (r == hipSuccess && (flags & TAROK_HISTORY)) r = hipMalloc((void **)&e->hist, (size_t)n_games * 48);
    if (r == hipSuccess && e->hist) r = hipMemset(e->hist, 255, (size_t)n_games * 48);
    size_t groups = (size_t)((n_games + TK_BLOCK - 1) / TK_BLOCK);
    if (r == hipSuccess) r = hipMalloc((void **)&e->rlist, groups * 2 * TK_REFILL_CAP * sizeof(u64));
    if (r == hipSuccess) r = hipMalloc((void **)&e->rcount, TK_RC(groups, 0) * sizeof(u32));
    if (r == hipSuccess) r = hipMalloc((void **)&e->elist, groups * 2 * TK_BULK_CAP * sizeof(u64));
    if (r == hipSuccess) r = hipMalloc((void **)&e->adam_sumsq, 1024 * sizeof(float));
    if (r == hipSuccess) r = hipMalloc((void **)&e->epoch, 2 * TK_EPOCH_WORDS * sizeof(u32));
    if (r == hipSuccess) r = hipMemset(e->epoch, 0, 2 * TK_EPOCH_WORDS * sizeof(u32));
    if (r == hipSuccess) r = hipMemset(e->rcount, 0, TK_RC(groups, 0) * sizeof(u32));
    if (r == hipSuccess) r = hipMemset(e->s01, 0, (size_t)n_games * sizeof(ulonglong2));
    if (r == hipSuccess) r = hipMemset(e->s23, 0, (size_t)n_games * sizeof(ulonglong2));
    if (r == hipSuccess) r = hipMemset(e->aux, 0, (size_t)n_games * sizeof(Aux));
    if (r == hipSuccess) r = hipMemset(e->cnt, 0, (size_t)n_games * sizeof(Counters));
    if (r == hipSuccess) r = hipMemset(e->nstale, 0, stale_bytes);
    if (r == hipSuccess) r = hipMemset(e->gkey, 0, (size_t)n_games * sizeof(u64));
    if (r == hipSuccess) r = hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking);
    if (r != hipSuccess) {
        g_last_hip = (int)r;
        tarok_destroy(e);
        return r == hipErrorOutOfMemory ? TAROK_ENOMEM : TAROK_EHIP;
    }
    *out = e;
    return TAROK_OK;
}

static void drop_graphs(tarok_env *e) {      // (behind a device synchronisation: nothing of theirs is queued any more)
    (void)hipDeviceSynchronize();
    for (int k = 0; k < e->n_graphs; k++) (void)hipGraphExecDestroy(e->graphs[k].exec);
    e->n_graphs = 0;
}

void tarok_destroy(tarok_env *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    drop_graphs(e);
    if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
    (void)hipFree(e->s01); (void)hipFree(e->s23); (void)hipFree(e->aux); (void)hipFree(e->cnt); (void)hipFree(e->nstale); (void)hipFree(e->gkey);
    (void)hipFree(e->rlist); (void)hipFree(e->rcount); (void)hipFree(e->elist); (void)hipFree(e->epoch); (void)hipFree(e->hist); (void)hipFree(e->adam_sumsq);
    (void)hipFree(e->bid_deal);
    delete e;
}

int64_t tarok_num_games(const tarok_env *e) { return e ? e->n : 0; }

int tarok_set_option(tarok_env *e, int option, int value) {
    if (!e) return TAROK_EINVAL;
    if (option == TAROK_OPT_REFILL_FAN && value >= 1 && value <= TK_REFILL_FAN) {
        if ((uint32_t)value != e->refill_fan && e->launched) {
            // The fan sets the step launches' grid, and the device-side launch counters count workgroups of ONE grid size
            // (launch_phase): behind launches of the old grid they would put workgroups of one launch into different
            // phases.  So the change waits for everything queued, restarts the counters and empties all four refill lists
            // of every group — their entries are only ever a hint: a line whose deal is dropped stays stale (its tag says
            // so) until its slot reaches it, deals that game in place and lists all its lines again.
            HIPCHK(hipSetDevice(e->device));
            HIPCHK(hipDeviceSynchronize());
            HIPCHK(hipMemset(e->epoch, 0, 2 * TK_EPOCH_WORDS * sizeof(u32)));
            HIPCHK(hipMemset(e->rcount, 0, TK_RC((e->n + TK_BLOCK - 1) / TK_BLOCK, 0) * sizeof(u32)));
        }
        e->refill_fan = (uint32_t)value;
    } else if (option == TAROK_OPT_LAZY_REFILL && (value == 0 || value == 1)) {
        // (safe between any two launches: with the option off every step launch empties the stretch lists unworked, so
        // there is nothing on them when it comes back on, and entries dropped when it goes off only leave stale lines)
        e->lazy_refill = (uint32_t)value;
    } else return TAROK_EINVAL;
    return TAROK_OK;      // (graphs instantiated for the old tuning stay cached under their own key: tarok_run_random)
}

int tarok_set_play_mode(tarok_env *e, float temperature, float epsilon) {
    if (!e || temperature != temperature || epsilon != epsilon) return TAROK_EINVAL;
    if (!(epsilon >= 0.f && epsilon <= 1.f)) return TAROK_EINVAL;
    if (temperature < 0.f || (temperature > 0.f && temperature < 1e-6f) || temperature > 1e6f) return TAROK_EINVAL;
    e->temperature = temperature; e->epsilon = epsilon;
    e->greedy = temperature == 0.f;
    e->inv_t = e->greedy ? 1.f : 1.0f / temperature;
    e->explore_thr = (uint32_t)floor((double)epsilon * 16777216.0);
    e->eps_p = (float)e->explore_thr * (1.0f / 16777216.0f);      // (exact: thr <= 2^24)
    e->mode_on = !(temperature == 1.f && epsilon == 0.f);
    return TAROK_OK;      // (no HIP call: the next launch reads it; a caller's captured graph keeps the kernel and the values it captured)
}

int tarok_get_play_mode(const tarok_env *e, float *temperature_out, float *epsilon_out) {
    if (!e) return TAROK_EINVAL;
    if (temperature_out) *temperature_out = e->temperature;
    if (epsilon_out) *epsilon_out = e->epsilon;
    return TAROK_OK;
}

static inline void launch_prefetch(tarok_env *e, hipStream_t s) {
    dim3 grid((unsigned)((e->n + TK_PF_SLOTS - 1) / TK_PF_SLOTS));
    hipLaunchKernelGGL(k_prefetch, grid, dim3(TK_BLOCK), 0, s, e->n, e->seed, e->offset, e->mix, e->aux, e->cnt, e->nstale);
}

int tarok_reset(tarok_env *e, uint32_t episode, const uint8_t *deals, const int8_t *contract, const int8_t *declarer,
                const int8_t *king_suit, const int8_t *talon_choice, const uint8_t *discards, int flags, void *stream) {
    if (!e) return TAROK_EINVAL;
    if ((talon_choice == nullptr) != (discards == nullptr)) return TAROK_EINVAL;
    if (contract && !declarer) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemsetAsync(e->rcount, 0, TK_RC((e->n + TK_BLOCK - 1) / TK_BLOCK, 0) * sizeof(u32), (hipStream_t)stream));
    hipLaunchKernelGGL(k_reset, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed, e->offset,
                       episode, e->mix, flags, deals, contract, declarer, king_suit, talon_choice, discards, e->s01,
                       e->s23, e->aux, e->cnt, e->nstale, e->gkey);
    launch_prefetch(e, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_prefetch(tarok_env *e, void *stream) {
    if (!e) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    launch_prefetch(e, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_exchange(tarok_env *e, const int8_t *talon_choice, const uint8_t *discards, void *stream) {
    if (!e || (talon_choice == nullptr) != (discards == nullptr)) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_exchange, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, talon_choice,
                       discards, e->s01, e->s23, e->gkey);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_legal_actions(tarok_env *e, uint64_t *obs_out, int8_t *seat_out, void *stream) {
    if (!e || !obs_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_legal, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->s01, e->s23,
                       (u64 *)obs_out, seat_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// the diagnostics buffer for a kernel that writes `words` of it, or NULL (none registered, or too small)
static inline u64 *stamps_for(const tarok_env *e, size_t words) { return (e->stamps && e->stamps_words >= words) ? e->stamps : nullptr; }

// One play launch: play workgroups + the refill workgroups that work the previous launch's lists off.
// cards = 1 (tarok_step, tarok_step_random): the one-card kernel k_step; more cards: the Bot-policy card loops
// of k_play_wide.
static inline void launch_play(tarok_env *e, bool random, int cards, int64_t stride, const uint8_t *action_in,
                               uint8_t *action_out, int16_t *reward, uint8_t *done, uint16_t *trick, uint64_t *obs,
                               int flags, hipStream_t s) {
    u32 groups = (u32)((e->n + TK_BLOCK - 1) / TK_BLOCK);
    u32 fan = e->refill_fan;
    dim3 grid(groups + (groups + fan - 1) / fan);
    e->launched = 1;
    if (cards == 1 && e->lazy_refill) grid = dim3(groups);     // kind 0 (launch_count): the step workgroups work their own lists off
    if (cards == 1) {
#define TK_LAUNCH_STEP(R, Z)                                                                                             \
    hipLaunchKernelGGL((k_step<R, Z>), grid, dim3(TK_BLOCK), 0, s, e->n, e->seed, e->offset, e->mix, flags, groups, e->epoch, \
                       fan, action_in, action_out, reward, done, trick, (u64 *)obs, e->hist, e->s01, e->s23, e->aux, e->cnt,  \
                       e->gkey, e->rlist, e->rcount, e->elist)
        if (e->lazy_refill) { if (random) TK_LAUNCH_STEP(true, true); else TK_LAUNCH_STEP(false, true); }
        else                { if (random) TK_LAUNCH_STEP(true, false); else TK_LAUNCH_STEP(false, false); }
#undef TK_LAUNCH_STEP
        return;
    }
#define TK_LAUNCH_PLAY(H)                                                                                              \
    hipLaunchKernelGGL((k_play_wide<H>), grid, dim3(TK_BLOCK), 0, s, e->n, e->seed, e->offset, e->mix, flags, cards, stride, \
                       groups, e->epoch, fan, action_out, reward, done, trick, (u64 *)obs, e->hist, e->s01,            \
                       e->s23, e->aux, e->cnt, e->gkey, e->rlist, e->rcount, stamps)
    u64 *stamps = stamps_for(e, 3 * (size_t)((e->n + 63) / 64));
    if (e->hist) TK_LAUNCH_PLAY(true); else TK_LAUNCH_PLAY(false);
#undef TK_LAUNCH_PLAY
}

int tarok_step(tarok_env *e, const uint8_t *action, int16_t *reward_out, uint8_t *done_out, uint16_t *trick_out,
               uint64_t *obs_out, int flags, void *stream) {
    if (!e || !action || !obs_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    launch_play(e, false, 1, e->n, action, nullptr, reward_out, done_out, trick_out, obs_out, flags, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// k_policy_x4 where the batch streams (from 2^21 games; at 65,536 games its four cards in a row are 0.4 us of latency more
// per launch than the one-game kernel, at 2^20 the two are equal: profiles/r03_ab_step.txt) and the caller's arrays
// allow its 16-byte loads and 2-byte stores (torch allocations do)
static inline void launch_policy(tarok_env *e, const uint64_t *obs, uint8_t *action, hipStream_t s) {
    if (e->n >= (1 << 21) && (((uintptr_t)obs & 15) | ((uintptr_t)action & 1)) == 0)
        hipLaunchKernelGGL(k_policy_x4, dim3((unsigned)((e->n + 4 * TK_BLOCK - 1) / (4 * TK_BLOCK))), dim3(TK_BLOCK), 0, s, e->n,
                           (const u64 *)obs, e->gkey, action);
    else
        hipLaunchKernelGGL(k_policy, grid_for(e->n), dim3(TK_BLOCK), 0, s, e->n, (const u64 *)obs, e->gkey, action);
}

int tarok_policy_random(tarok_env *e, const uint64_t *obs, uint8_t *action_out, void *stream) {
    if (!e || !obs || !action_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    launch_policy(e, obs, action_out, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_step_random(tarok_env *e, uint8_t *action_out, int16_t *reward_out, uint8_t *done_out, uint16_t *trick_out,
                      uint64_t *obs_out, int flags, void *stream) {
    if (!e || !obs_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    launch_play(e, true, 1, e->n, nullptr, action_out, reward_out, done_out, trick_out, obs_out, flags, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_krog_random(tarok_env *e, int cards, int64_t stride, uint8_t *action_out, int16_t *reward_out,
                      uint8_t *done_out, uint16_t *trick_out, uint64_t *obs_out, int flags, void *stream) {
    if (!e || !obs_out || cards < 1 || cards > TAROK_MAX_CARDS_PER_LAUNCH || stride < e->n) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    launch_play(e, true, cards, stride, nullptr, action_out, reward_out, done_out, trick_out, obs_out, flags,
                (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// cards: 0 = tarok_policy_random + tarok_step, 1 = tarok_step_random, >= 2 = tarok_krog_random
static inline void launch_one(tarok_env *e, int cards, uint8_t *action, int16_t *reward, uint8_t *done,
                              uint64_t *obs, int flags, hipStream_t s) {
    if (cards >= 1) {
        launch_play(e, true, cards, e->n, nullptr, cards >= 2 ? action : nullptr, reward, done, nullptr, obs, flags, s);
    } else {
        launch_policy(e, obs, action, s);
        launch_play(e, false, 1, e->n, action, nullptr, reward, done, nullptr, obs, flags, s);
    }
}

int tarok_run_random(tarok_env *e, int64_t n_steps, int cards_per_launch, int graph_chunk, int prefetch_every,
                     uint8_t *action, int16_t *reward_out, uint8_t *done_out, uint64_t *obs_out, int flags, void *stream) {
    if (!e || !obs_out || n_steps < 0 || graph_chunk < 0 || graph_chunk > 8192 || prefetch_every < 0) return TAROK_EINVAL;
    if (cards_per_launch < 0 || cards_per_launch > TAROK_MAX_CARDS_PER_LAUNCH) return TAROK_EINVAL;
    int unit = cards_per_launch >= 2 ? cards_per_launch : 1;          // lock-steps per launch
    if (n_steps % unit != 0 || graph_chunk % unit != 0) return TAROK_EINVAL;
    if (prefetch_every % unit != 0) return TAROK_EINVAL;
    if (graph_chunk > 0 && prefetch_every > 0 && graph_chunk % prefetch_every != 0) return TAROK_EINVAL;
    if (!(flags & TAROK_AUTO_RESET)) prefetch_every = 0;
    if (cards_per_launch == 0 && !action) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    int64_t left = n_steps;
    if (graph_chunk > 0 && left >= graph_chunk) {
        hipGraphExec_t gexec = nullptr;
        for (int k = 0; k < e->n_graphs && !gexec; k++) {
            const tarok_env::GraphEntry &g = e->graphs[k];
            if (g.fused == cards_per_launch && g.chunk == graph_chunk && g.flags == flags && g.prefetch == prefetch_every &&
                g.action == action && g.reward == reward_out && g.done == done_out && g.obs == obs_out && g.stamps == e->stamps &&
                g.fan == e->refill_fan && g.lazy == e->lazy_refill)
                gexec = g.exec;
        }
        if (!gexec) {
            if (e->n_graphs == TK_GRAPH_CACHE) drop_graphs(e);
            hipGraph_t graph = nullptr;
            HIPCHK(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeRelaxed));
            for (int k = 0; k < graph_chunk; k += unit) {
                launch_one(e, cards_per_launch, action, reward_out, done_out, obs_out, flags, e->cap_stream);
                if (prefetch_every && (k + unit) % prefetch_every == 0) launch_prefetch(e, e->cap_stream);
            }
            HIPCHK(hipStreamEndCapture(e->cap_stream, &graph));
            hipError_t r = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (r != hipSuccess) { g_last_hip = (int)r; return TAROK_EHIP; }
            e->graphs[e->n_graphs++] = {gexec, cards_per_launch, graph_chunk, flags, prefetch_every, action, reward_out, done_out,
                                        obs_out, e->stamps, e->refill_fan, e->lazy_refill};
        }
        while (left >= graph_chunk) {
            HIPCHK(hipGraphLaunch(gexec, s));
            left -= graph_chunk;
        }
    }
    for (int64_t k = 0; left > 0; left -= unit, k += unit) {
        launch_one(e, cards_per_launch, action, reward_out, done_out, obs_out, flags, s);
        if (prefetch_every && (k + unit) % prefetch_every == 0) launch_prefetch(e, s);
    }
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_rollout_random(tarok_env *e, uint32_t episode, int16_t *scores_out, int16_t *nsteps_out, int8_t *seats_out,
                         uint64_t *masks_out, uint8_t *actions_out, void *stream) {
    if (!e) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_rollout, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed, e->offset,
                       episode, e->mix, scores_out, nsteps_out, seats_out, (u64 *)masks_out, actions_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

extern "C++" {
// Lanes per game of a playout launch, as lg: a power of two near four per playout of a row (a mover has 1..12 legal cards,
// followers few), 2^min_lg .. 256.  4 * worlds <= lanes, so the worlds of a workgroup's teams fit its TK_PO_WORLD_SLOTS slots.
static_assert(TAROK_PLAYOUT_MAX_WORLDS * 4 <= TK_BLOCK && TK_PO_WORLD_SLOTS * 4 == TK_BLOCK, "teams * worlds <= TK_PO_WORLD_SLOTS");
static inline u32 playout_lg(u32 min_lg, int playouts) {
    u32 lg = min_lg;
    while (lg < TK_PO_MAX_LG && (1 << lg) < 4 * playouts) lg++;
    return lg;
}
static inline dim3 playout_grid(const tarok_env *e, u32 lg) {
    const int64_t teams = TK_BLOCK >> lg;
    return dim3((unsigned)((e->n + teams - 1) / teams));
}

// The arguments every playout launch takes (an open-hand launch has one world).
static inline bool playout_args_ok(const tarok_env *e, int worlds, int samples, int seats) {
    return e && worlds >= 1 && worlds <= TAROK_PLAYOUT_MAX_WORLDS && samples >= 1 && samples <= TAROK_PLAYOUT_MAX_SAMPLES && seats >= 0 &&
           seats <= 15;
}

// One card launch.  WORLDS: the kernel takes (worlds, samples); else samples alone, and `worlds` is 1.  `words`: the
// dealer's per-game words, where it has any.
template <bool WORLDS, class Kernel, class... Words>
static int launch_playout_cards(Kernel kernel, tarok_env *e, int worlds, int samples, uint64_t salt, int seats,
                                const uint8_t *seats_per_game, int32_t *sum_out, uint8_t *action_out, void *stream, Words... words) {
    if (!playout_args_ok(e, worlds, samples, seats) || (!sum_out && !action_out) || (... || !words)) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    const u32 lg = playout_lg(TK_PO_MIN_LG, worlds * samples);
    auto launch = [&](auto... counts) {
        hipLaunchKernelGGL(kernel, playout_grid(e, lg), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed ^ (u64)salt, e->offset,
                           counts..., lg, (u32)seats, seats_per_game, e->s01, e->s23, e->cnt, e->gkey, words...,
                           reinterpret_cast<int4 *>(sum_out), action_out);
    };
    if constexpr (WORLDS) launch((u32)worlds, (u32)samples); else launch((u32)samples);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// A halving schedule as the host reads it: the rounds' world counts, their cumulative ends — also packed a byte a round, as
// the Bot-played kernels take them — and the total.
struct HalvingSchedule {
    int rounds = 0, worlds = 0;
    int w[TAROK_PLAYOUT_MAX_ROUNDS] = {0, 0, 0, 0}, end[TAROK_PLAYOUT_MAX_ROUNDS] = {0, 0, 0, 0};
    u32 ends = 0;
};
// false: rounds outside 1..TAROK_PLAYOUT_MAX_ROUNDS, a NULL schedule, a count < 1 or a sum above TAROK_PLAYOUT_MAX_WORLDS.
static bool halving_schedule(int rounds, const int *round_worlds, HalvingSchedule &h) {
    if (rounds < 1 || rounds > TAROK_PLAYOUT_MAX_ROUNDS || !round_worlds) return false;
    h.rounds = rounds;
    for (int r = 0; r < rounds; r++) {
        if (round_worlds[r] < 1 || round_worlds[r] > TAROK_PLAYOUT_MAX_WORLDS - h.worlds) return false;
        h.w[r] = round_worlds[r];
        h.end[r] = h.worlds += round_worlds[r];
        h.ends |= (u32)h.worlds << (8 * r);
    }
    return true;
}

// One halving launch: the schedule goes to the kernel as its cumulative ends, a byte a round; lg is the card launches' at
// (all worlds) x samples, so the team's worlds fit its slots.  `words`: the dealer's per-game words (a typed null for the
// det kind).
template <class Kernel, class Word>
static int launch_playout_halving(Kernel kernel, tarok_env *e, int rounds, const int *round_worlds, int samples, uint64_t salt, int seats,
                                  const uint8_t *seats_per_game, int32_t *sum_out, int32_t *count_out, uint8_t *action_out, void *stream,
                                  const Word *words) {
    HalvingSchedule h;
    if (!halving_schedule(rounds, round_worlds, h) || !playout_args_ok(e, h.worlds, samples, seats) ||
        (!sum_out && !count_out && !action_out))
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    const u32 lg = playout_lg(TK_PO_MIN_LG, h.worlds * samples);
    hipLaunchKernelGGL(kernel, playout_grid(e, lg), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed ^ (u64)salt, e->offset, h.ends,
                       (u32)samples, lg, (u32)seats, seats_per_game, e->s01, e->s23, e->cnt, e->gkey, words,
                       reinterpret_cast<int4 *>(sum_out), reinterpret_cast<int4 *>(count_out), action_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// The world kind of a launch that takes (kind, words): f(the kind as an integral constant, the words as the kind's type —
// a typed null for DET, whose dealer reads none).  The caller has checked the kind's range and what it asks of `words`.
template <class F>
static int for_world_kind(int kind, const void *words, F f) {
    if (kind == TAROK_NET_WORLDS_VOIDS) return f(std::integral_constant<int, TAROK_NET_WORLDS_VOIDS>{}, (const u32 *)words);
    if (kind == TAROK_NET_WORLDS_HIDDEN) return f(std::integral_constant<int, TAROK_NET_WORLDS_HIDDEN>{}, (const u64 *)words);
    return f(std::integral_constant<int, TAROK_NET_WORLDS_DET>{}, (const NoWord *)nullptr);
}
// A kernel family's member of for_world_kind's kind K: one row per family, in TAROK_NET_WORLDS_* order.
#define TK_OF_KIND(K, DET, VOIDS, HIDDEN) std::get<decltype(K)::value>(std::make_tuple(DET, VOIDS, HIDDEN))
static inline bool world_kind_ok(int kind) { return kind >= TAROK_NET_WORLDS_DET && kind <= TAROK_NET_WORLDS_HIDDEN; }

// tarok_playout_bids and its _pass twin: the deal, then the playout kernel given
template <class Kernel>
static int launch_playout_bids(Kernel kernel, tarok_env *e, uint32_t episode, const uint8_t *deals, int worlds, int samples, int contracts,
                               uint64_t salt, int seats, const uint8_t *seats_per_game, int32_t *sum_out, void *stream) {
    if (!playout_args_ok(e, worlds, samples, seats) || contracts < 1 || contracts > TAROK_BID_ALL_CONTRACTS) return TAROK_EINVAL;
    if (!sum_out) return TAROK_OK;
    HIPCHK(hipSetDevice(e->device));
    if (!e->bid_deal) HIPCHK(hipMalloc((void **)&e->bid_deal, (size_t)e->n * 5 * sizeof(u64)));   // on the first call; tarok_destroy frees it
    hipLaunchKernelGGL(k_bid_deal, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed, e->offset, episode, deals, e->bid_deal);
    // 16 lanes per game or more, so a workgroup's at most 16 teams keep their 80 sums each in 5 KiB
    static_assert(TAROK_BID_ROWS == TK_BID_ROWS && TAROK_BID_ROWS % 4 == 0, "a viewer's rows are whole 16-byte pieces");
    static_assert(TAROK_BID_PASS_ROW == TK_BID_PASS_ROW && TK_BID_PASS_ROW == TK_BID_OPTIONS && TK_BID_PASS_ROW < 32, "row 19, in the key's five bits");
    const u32 lg = playout_lg(TK_PB_MIN_LG, worlds * samples);
    hipLaunchKernelGGL(kernel, playout_grid(e, lg), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed ^ (u64)salt, e->offset, episode, (u32)worlds, (u32)samples, lg, (u32)contracts, (u32)seats, seats_per_game,
                       e->bid_deal, reinterpret_cast<int4 *>(sum_out));
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// ---- the net-played launches: what the dense and the list entries share
#define TK_WEIGHTS(w1, b1, w2, b2, w3, b3) PolicyWeights{(const __bf16 *)(w1), b1, (const __bf16 *)(w2), b2, (const __bf16 *)(w3), b3}

// The four item arrays of a net launch in its scratch (tarok_playout_cards_net's layout).
struct NetItems {
    ulonglong2 *i01, *i23;
    u64 *ikey, *ires;
    NetItems(void *scratch, int64_t items)
        : i01(reinterpret_cast<ulonglong2 *>(scratch)), i23(i01 + items), ikey(reinterpret_cast<u64 *>(i23 + items)), ires(ikey + items) {}
};
static inline bool net_args_ok(int net_seats, const PolicyWeights &w, const void *scratch, int64_t scratch_bytes, int64_t need) {
    return net_seats >= 0 && net_seats <= 15 && w.w1 && w.b1 && w.w2 && w.b2 && w.w3 && w.b3 && scratch && !((uintptr_t)scratch & 15) &&
           need >= 0 && scratch_bytes >= need;
}
// What an entry takes of depth and value_scale: lo..hi — each entry point states its own range — and a finite value_scale > 0.
static inline bool depth_args_ok(int depth, int lo, int hi, float value_scale) {
    return depth >= lo && depth <= hi && value_scale > 0.f && !__builtin_isinf(value_scale);
}

// The play launch over a net launch's items, the one place that picks among the four play kernels.  total NULL: the dense
// layout, `items` the host's count; else the compacted list, whose count is the device's total word and `items` the host's
// bound: the grid is the bound's (one workgroup where the bound is 0: it finds no row below the total).  depth = 0: to the
// last card; else the _value kernel, whose live items carry their viewers (the caller's item kernel is the _value form).
// b non-NULL: the VERSUS kernels (tarok_playout_cards_net_versus) — w is network A, *b network B, own_rel / opp_rel the role
// sets over the seats relative to each item's viewer, net_seats is not read, and the caller's item kernel is the _value form
// at every depth.  modes non-NULL (with b, dense only: tarok_playout_cards_net_sampled): the SAMPLED kernels, modes[0] network A's
// play mode and modes[1] network B's.
static inline void launch_net_play(int64_t items, const u32 *total, int net_seats, const NetItems &it, const PolicyWeights &w,
                                   hipStream_t s, int depth, float value_scale, const PolicyWeights *b = nullptr, int own_rel = 0,
                                   int opp_rel = 0, const PlayMode *modes = nullptr) {
    const int64_t tiles = net_list_tiles(items, PM_M);
    const dim3 grid((unsigned)(tiles ? tiles : 1));
#define TK_LAUNCH_NET_PLAY(K, COUNT, ...)                                                                                          \
    hipLaunchKernelGGL(K, grid, dim3(TK_BLOCK), 0, s, COUNT, (u32)net_seats, it.i01, it.i23, it.ikey, it.ires, w.w1, w.b1, w.w2, \
                       w.b2, w.w3, w.b3, ##__VA_ARGS__)
    if (b) {
        net_seats = own_rel;                             // (the VERSUS kernels take own_rel where the others take net_seats)
        if (modes) {
#define TK_MODES modes[0].inv_t, modes[0].greedy, modes[0].thr, modes[0].eps, modes[1].inv_t, modes[1].greedy, modes[1].thr, modes[1].eps
            if (depth) TK_LAUNCH_NET_PLAY(k_playout_net_play_sampled_value, items, (u32)opp_rel, *b, TK_MODES, (u32)depth, value_scale);
            else TK_LAUNCH_NET_PLAY(k_playout_net_play_sampled, items, (u32)opp_rel, *b, TK_MODES);
#undef TK_MODES
        } else if (total) {
            if (depth) TK_LAUNCH_NET_PLAY(k_playout_net_play_list_versus_value, total, (u32)opp_rel, *b, (u32)depth, value_scale);
            else TK_LAUNCH_NET_PLAY(k_playout_net_play_list_versus, total, (u32)opp_rel, *b);
        } else {
            if (depth) TK_LAUNCH_NET_PLAY(k_playout_net_play_versus_value, items, (u32)opp_rel, *b, (u32)depth, value_scale);
            else TK_LAUNCH_NET_PLAY(k_playout_net_play_versus, items, (u32)opp_rel, *b);
        }
    } else if (total) {
        if (depth) TK_LAUNCH_NET_PLAY(k_playout_net_play_list_value, total, (u32)depth, value_scale);
        else TK_LAUNCH_NET_PLAY(k_playout_net_play_list, total);
    } else {
        if (depth) TK_LAUNCH_NET_PLAY(k_playout_net_play_value, items, (u32)depth, value_scale);
        else TK_LAUNCH_NET_PLAY(k_playout_net_play, items);
    }
#undef TK_LAUNCH_NET_PLAY
}

// One net card launch: the items (`deal`, the dealer's kernel, with its per-game `words`: a typed null for a det kernel,
// which takes none), the playouts, the sums — three launches on `stream`, nothing allocated.  depth = 0: the playouts run
// to the last card; else (checked by tarok_playout_cards_net_value, the only caller that gives one) they stop at the
// viewer's depth-th decision, and `deal` is a k_playout_net_deal_value*.  b non-NULL (tarok_playout_cards_net_versus, which has
// checked the roles): launch_net_play's VERSUS form, `deal` a k_playout_net_deal_value* at every depth.
// SAMPLED (tarok_playout_cards_net_sampled, which has checked the roles and made the modes): `deal` is a
// k_playout_net_deal_sampled*, which takes `samples` last; the items are (rank, world, sample), the scratch
// tarok_playout_cards_net_sampled_scratch's, the play launch the SAMPLED kernels under modes[0..1], and k_playout_net_sum sums a
// row's worlds x samples contiguous items.  The team layout (lg) stays the worlds'.
template <bool SAMPLED = false, class Kernel, class Word>
static int launch_playout_cards_net(Kernel deal, tarok_env *e, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                    const Word *words, int net_seats, const PolicyWeights &w, void *scratch, int64_t scratch_bytes,
                                    int32_t *sum_out, uint8_t *action_out, void *stream, int depth, float value_scale,
                                    const PolicyWeights *b = nullptr, int own_rel = 0, int opp_rel = 0, int samples = 1,
                                    const PlayMode *modes = nullptr) {
    constexpr bool has_words = !std::is_same<Word, NoWord>::value;
    if (!playout_args_ok(e, worlds, samples, seats) ||
        !net_args_ok(net_seats, w, scratch, scratch_bytes,
                     SAMPLED ? tarok_playout_cards_net_sampled_scratch(e, worlds, samples) : tarok_playout_net_scratch(e, worlds)) ||
        (!sum_out && !action_out) || (has_words && !words))
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    const int64_t items = e->n * TAROK_PLAYOUT_RANKS * (int64_t)worlds * (int64_t)samples;
    const NetItems it(scratch, items);
    const u32 lg = playout_lg(TK_PO_MIN_LG, worlds);
    auto launch_deal = [&](auto... kwords) {
        if constexpr (SAMPLED)
            hipLaunchKernelGGL(deal, playout_grid(e, lg), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed ^ (u64)salt, e->offset,
                               (u32)worlds, lg, (u32)seats, seats_per_game, e->s01, e->s23, e->cnt, kwords..., it.i01, it.i23, it.ikey,
                               it.ires, (u32)samples);
        else
            hipLaunchKernelGGL(deal, playout_grid(e, lg), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed ^ (u64)salt, e->offset,
                               (u32)worlds, lg, (u32)seats, seats_per_game, e->s01, e->s23, e->cnt, kwords..., it.i01, it.i23, it.ikey,
                               it.ires);
    };
    if constexpr (has_words) launch_deal(words); else launch_deal();
    launch_net_play(items, nullptr, net_seats, it, w, (hipStream_t)stream, depth, value_scale, b, own_rel, opp_rel, SAMPLED ? modes : nullptr);
    hipLaunchKernelGGL(k_playout_net_sum, dim3((unsigned)((e->n + 15) / 16)), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n,
                       (u32)(worlds * samples), (u32)seats, seats_per_game, e->s01, e->s23, e->gkey, it.ires,
                       reinterpret_cast<int4 *>(sum_out), action_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// tarok_playout_exchange_net and its _value twin: the items, the playouts, the sums and the choice — three launches on `stream`,
// nothing allocated.  depth = 0: the playouts run to the last card; else (checked by tarok_playout_exchange_net_value, the only
// caller that gives one) they stop at the declarer's depth-th decision.
static int launch_playout_exchange_net(tarok_env *e, int worlds, int discard_sets, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                       int net_seats, const PolicyWeights &w, void *scratch, int64_t scratch_bytes, int32_t *sum_out,
                                       int8_t *choice_out, uint8_t *discards_out, void *stream, int depth, float value_scale) {
    if (!playout_args_ok(e, worlds, 1, seats) || discard_sets < 1 || discard_sets > TAROK_EXCHANGE_MAX_SETS ||
        !net_args_ok(net_seats, w, scratch, scratch_bytes, tarok_playout_exchange_net_scratch(e, worlds, discard_sets)) ||
        (!sum_out && !choice_out && !discards_out))
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    const int64_t items = e->n * 6 * (int64_t)discard_sets * (int64_t)worlds;
    const NetItems it(scratch, items);
    const u32 lg = playout_lg(TK_PX_MIN_LG, worlds);     // tarok_playout_exchange's teams at samples = 1
    hipLaunchKernelGGL(depth ? k_playout_exchange_net_deal_value : k_playout_exchange_net_deal, playout_grid(e, lg), dim3(TK_BLOCK), 0,
                       (hipStream_t)stream, e->n, items, e->seed ^ (u64)salt, e->offset, (u32)worlds, (u32)discard_sets, lg, (u32)seats,
                       seats_per_game, e->s01, e->s23, e->cnt, it.i01, it.i23, it.ikey, it.ires);
    launch_net_play(items, nullptr, net_seats, it, w, (hipStream_t)stream, depth, value_scale);
    hipLaunchKernelGGL(k_playout_exchange_net_sum, dim3((unsigned)((e->n + 15) / 16)), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, items,
                       e->seed ^ (u64)salt, e->offset, (u32)worlds, (u32)discard_sets, (u32)seats, seats_per_game, e->s01, e->s23, e->cnt,
                       e->gkey, it.ires, reinterpret_cast<int4 *>(sum_out), choice_out, discards_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// tarok_playout_bids_net and its _value twin: the deal, the items, the playouts, the sums — four launches on `stream`, nothing
// allocated.  depth = 0: the playouts run to the last card and `pass` is 0; else (checked by tarok_playout_bids_net_value, the
// only caller that gives one) they stop at the viewer's depth-th decision, and pass = 1 makes row 19's slots items.
static int launch_playout_bids_net(tarok_env *e, uint32_t episode, const uint8_t *deals, int worlds, int contracts, uint64_t salt, int seats,
                                   const uint8_t *seats_per_game, int net_seats, const PolicyWeights &w, void *scratch,
                                   int64_t scratch_bytes, int32_t *sum_out, void *stream, int depth, float value_scale, int pass) {
    if (!playout_args_ok(e, worlds, 1, seats) || contracts < 1 || contracts > TAROK_BID_ALL_CONTRACTS ||
        !net_args_ok(net_seats, w, scratch, scratch_bytes, tarok_playout_bids_net_scratch(e, worlds)) || !sum_out)
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    const int64_t rows = e->n * 4 * TAROK_BID_ROWS, items = rows * (int64_t)worlds;
    const NetItems it(scratch, items);
    u64 *deal = it.ires + items;
    hipLaunchKernelGGL(k_bid_deal, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed, e->offset, episode, deals, deal);
    const u32 lg = playout_lg(TK_PB_MIN_LG, worlds);     // tarok_playout_bids' teams at samples = 1
    hipLaunchKernelGGL(!depth ? k_playout_bids_net_deal : (pass ? k_playout_bids_net_deal_value_pass : k_playout_bids_net_deal_value),
                       playout_grid(e, lg), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, items, e->seed ^ (u64)salt, e->offset, episode,
                       (u32)worlds, lg, (u32)contracts, (u32)seats, seats_per_game, deal, it.i01, it.i23, it.ikey, it.ires);
    launch_net_play(items, nullptr, net_seats, it, w, (hipStream_t)stream, depth, value_scale);
    hipLaunchKernelGGL(k_playout_bids_net_sum, grid_for(rows), dim3(TK_BLOCK), 0, (hipStream_t)stream, rows, items, (u32)worlds, it.ires,
                       sum_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// The scratch of a list launch, layout and size from the same offsets: the four item arrays at the bound (NetItems), `extra`
// bytes of the launch's own, per unit the on word and `more` further words (halving's alive), per unit the base word, the
// scan's partials (a word per TK_BLOCK units) and the total word, rounded up to 16.
struct ListArrays : NetItems {
    char *extra;
    u32 *on, *base, *part, *total;
};
struct ListScratch {
    int64_t units = 0, bound = 0, blocks = 0, extra = 0, more = 0, bytes = 0;
    int64_t on_at() const { return bound * TK_PN_ITEM_BYTES + extra; }
    int64_t base_at() const { return on_at() + (1 + more) * units * 4; }
    int64_t total_at() const { return base_at() + (units + blocks) * 4; }
    // false: a bound that reaches 2^31 items (the list's slots are 32-bit words)
    bool plan(int64_t units_, int64_t bound_, int64_t extra_, int64_t more_ = 0) {
        if (bound_ >= (1LL << 31)) return false;
        units = units_, bound = bound_, extra = extra_, more = more_;
        blocks = (units + TK_BLOCK - 1) / TK_BLOCK;
        bytes = (total_at() + 4 + 15) & ~(int64_t)15;
        return true;
    }
    ListArrays carve(void *scratch) const {
        char *s = reinterpret_cast<char *>(scratch);
        u32 *base = reinterpret_cast<u32 *>(s + base_at());
        return ListArrays{NetItems(scratch, bound), s + on_at() - extra, reinterpret_cast<u32 *>(s + on_at()), base, base + units,
                          reinterpret_cast<u32 *>(s + total_at())};
    }
};
// The list's prefix sum over the units' on words at `worlds` items each: base[u] and the total word.
static inline void launch_list_scan(const ListScratch &p, const ListArrays &a, int worlds, hipStream_t s) {
    hipLaunchKernelGGL(k_playout_net_list_totals, grid_for(p.units), dim3(TK_BLOCK), 0, s, p.units, (u32)worlds, a.on, a.part);
    hipLaunchKernelGGL(k_playout_net_list_scan, dim3(1), dim3(TK_BLOCK), 0, s, (u32)p.blocks, a.part, a.total);
    hipLaunchKernelGGL(k_playout_net_list_base, grid_for(p.units), dim3(TK_BLOCK), 0, s, p.units, (u32)worlds, a.on, a.part, a.base);
}
// The front lists' items in the worlds e0 .. e0 + round_worlds - 1, the one place per family that picks among the deal kernels:
// the list entries' single launch is e0 = 0 over all their worlds at the list's bound, a halving round its own worlds and bound.
static inline void launch_exchange_list_deal(tarok_env *e, const ListArrays &a, int64_t bound, u64 pseed, int e0, int round_worlds,
                                             int discard_sets, int seats, const uint8_t *seats_per_game, int depth, hipStream_t s) {
    const u32 lg = playout_lg(TK_PX_MIN_LG, round_worlds);      // tarok_playout_exchange's teams at samples = 1
    hipLaunchKernelGGL(depth ? k_playout_exchange_net_list_deal_value : k_playout_exchange_net_list_deal, playout_grid(e, lg), dim3(TK_BLOCK),
                       0, s, e->n, (u32)bound, pseed, e->offset, (u32)e0, (u32)round_worlds, (u32)discard_sets, lg, (u32)seats, seats_per_game,
                       e->s01, e->s23, e->cnt, a.on, a.base, a.i01, a.i23, a.ikey, a.ires);
}
static inline void launch_bids_list_deal(tarok_env *e, const ListArrays &a, int64_t bound, u64 pseed, uint32_t episode, int e0,
                                         int round_worlds, int seats, const uint8_t *seats_per_game, const u64 *deal, int depth,
                                         int pass_value, hipStream_t s) {
    const u32 lg = playout_lg(TK_PB_MIN_LG, round_worlds);      // tarok_playout_bids' teams at samples = 1
    hipLaunchKernelGGL(!depth ? k_playout_bids_net_list_deal
                              : (pass_value ? k_playout_bids_net_list_deal_value_pass : k_playout_bids_net_list_deal_value),
                       playout_grid(e, lg), dim3(TK_BLOCK), 0, s, e->n, (u32)bound, pseed, e->offset, episode, (u32)e0, (u32)round_worlds, lg,
                       (u32)seats, seats_per_game, deal, a.on, a.base, a.i01, a.i23, a.ikey, a.ires);
}

// A net halving launch as the host sizes it: the schedule, and the list at the largest round's bound over the games as units.
// Its extension of the list's layout: a game's running sums (16 bytes a rank) and counts (4) are the extra bytes, its alive
// word follows its on word.  false: a NULL env, a schedule halving_schedule refuses, or a round whose bound reaches 2^31.
struct NetHalvingPlan {
    HalvingSchedule h;
    ListScratch list;
};
static bool net_halving_plan(const tarok_env *e, int rounds, const int *round_worlds, NetHalvingPlan &p) {
    if (!e || !halving_schedule(rounds, round_worlds, p.h)) return false;
    int64_t bound = 0;
    for (int r = 0; r < rounds; r++) {
        const int64_t b = net_list_bound(e->n, (u32)r, (u32)p.h.w[r]);
        bound = b > bound ? b : bound;
    }
    return p.list.plan(e->n, bound, e->n * TAROK_PLAYOUT_RANKS * (int64_t)(sizeof(int4) + sizeof(int)), 1);
}
// The front list launches as the host sizes them: the exchange's units are (game, group), the bids' (game, viewer), whose
// extra bytes are k_bid_deal's 40 per game.
static bool exchange_list_plan(const tarok_env *e, int worlds, int discard_sets, ListScratch &p) {
    if (!e || worlds < 1 || worlds > TAROK_PLAYOUT_MAX_WORLDS || discard_sets < 1 || discard_sets > TAROK_EXCHANGE_MAX_SETS) return false;
    return p.plan(e->n * 6, exchange_list_bound(e->n, (u32)discard_sets, (u32)worlds), 0);
}
static bool bid_list_plan(const tarok_env *e, int worlds, int contracts, int seats, int per_game_seats, int pass_value, ListScratch &p) {
    if (!e || worlds < 1 || worlds > TAROK_PLAYOUT_MAX_WORLDS || contracts < 1 || contracts > TAROK_BID_ALL_CONTRACTS || seats < 0 ||
        seats > 15 || per_game_seats < 0 || per_game_seats > 1 || pass_value < 0 || pass_value > 1)
        return false;
    return p.plan(e->n * 4, bid_list_bound(e->n, (u32)seats, per_game_seats != 0, (u32)contracts, (u32)pass_value, (u32)worlds),
                  e->n * 5 * (int64_t)sizeof(u64));
}
// The front halving launches as the host sizes them: the schedule, each round's bound B_r (the play grid's) and the list at
// B = max B_r over the list launches' units, with an alive word after each on word.  The extra bytes: a row's running sums
// and count — 16 + 4 bytes for each of the exchange's 6 D rows, 4 + 4 for each of the bids' 4 x 20 — and then the bids' deal.
// false: what the list plans and halving_schedule refuse, or a round whose bound reaches 2^31.
struct FrontHalvingPlan {
    HalvingSchedule h;
    ListScratch list;
    int64_t round_bound[TAROK_PLAYOUT_MAX_ROUNDS] = {0, 0, 0, 0};
    template <class Bound> bool plan(int64_t units, int64_t extra, Bound bound_of) {
        int64_t bound = 0;
        for (int r = 0; r < h.rounds; r++) {
            round_bound[r] = bound_of((u32)r, (u32)h.w[r]);
            if (round_bound[r] >= (1LL << 31)) return false;
            bound = round_bound[r] > bound ? round_bound[r] : bound;
        }
        return list.plan(units, bound, extra, 1);
    }
};
static bool exchange_halving_plan(const tarok_env *e, int rounds, const int *round_worlds, int discard_sets, FrontHalvingPlan &p) {
    if (!e || !halving_schedule(rounds, round_worlds, p.h) || discard_sets < 1 || discard_sets > TAROK_EXCHANGE_MAX_SETS) return false;
    return p.plan(e->n * 6, e->n * 6 * (int64_t)discard_sets * (int64_t)(sizeof(int4) + sizeof(int)),
                  [&](u32 r, u32 wr) { return exchange_halving_bound(e->n, (u32)discard_sets, r, wr); });
}
static bool bid_halving_plan(const tarok_env *e, int rounds, const int *round_worlds, int contracts, int seats, int per_game_seats,
                             int pass_value, FrontHalvingPlan &p) {
    if (!e || !halving_schedule(rounds, round_worlds, p.h) || contracts < 1 || contracts > TAROK_BID_ALL_CONTRACTS || seats < 0 ||
        seats > 15 || per_game_seats < 0 || per_game_seats > 1 || pass_value < 0 || pass_value > 1)
        return false;
    return p.plan(e->n * 4, e->n * 4 * TAROK_BID_ROWS * (int64_t)(2 * sizeof(int)) + e->n * 5 * (int64_t)sizeof(u64), [&](u32 r, u32 wr) {
        return bid_halving_bound(e->n, (u32)seats, per_game_seats != 0, (u32)contracts, (u32)pass_value, r, wr);
    });
}
}

int tarok_playout_cards(tarok_env *e, int samples, uint64_t salt, int seats, const uint8_t *seats_per_game, int32_t *sum_out,
                        uint8_t *action_out, void *stream) {
    return launch_playout_cards<false>(k_playout, e, 1, samples, salt, seats, seats_per_game, sum_out, action_out, stream);
}

int tarok_playout_cards_det(tarok_env *e, int worlds, int samples, uint64_t salt, int seats, const uint8_t *seats_per_game,
                            int32_t *sum_out, uint8_t *action_out, void *stream) {
    return launch_playout_cards<true>(k_playout_det, e, worlds, samples, salt, seats, seats_per_game, sum_out, action_out, stream);
}

int64_t tarok_playout_net_scratch(const tarok_env *e, int worlds) {
    if (!e || worlds < 1 || worlds > TAROK_PLAYOUT_MAX_WORLDS) return TAROK_EINVAL;
    return e->n * TAROK_PLAYOUT_RANKS * (int64_t)worlds * TK_PN_ITEM_BYTES;
}

// (the plain dense entries take no depth and no value_scale: nothing of either is looked at)
int tarok_playout_cards_net(tarok_env *e, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game, int net_seats,
                            const void *w1, const float *b1, const void *w2, const float *b2, const void *w3, const float *b3,
                            void *scratch, int64_t scratch_bytes, int32_t *sum_out, uint8_t *action_out, void *stream) {
    return launch_playout_cards_net(k_playout_net_deal, e, worlds, salt, seats, seats_per_game, (const NoWord *)nullptr, net_seats,
                                    TK_WEIGHTS(w1, b1, w2, b2, w3, b3), scratch, scratch_bytes, sum_out, action_out, stream, 0, 0.f);
}

int tarok_playout_cards_net_voids(tarok_env *e, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                  const uint32_t *voids, int net_seats, const void *w1, const float *b1, const void *w2, const float *b2,
                                  const void *w3, const float *b3, void *scratch, int64_t scratch_bytes, int32_t *sum_out,
                                  uint8_t *action_out, void *stream) {
    return launch_playout_cards_net(k_playout_net_deal_voids, e, worlds, salt, seats, seats_per_game, voids, net_seats,
                                    TK_WEIGHTS(w1, b1, w2, b2, w3, b3), scratch, scratch_bytes, sum_out, action_out, stream, 0, 0.f);
}

int tarok_playout_cards_net_hidden(tarok_env *e, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                   const uint64_t *played, int net_seats, const void *w1, const float *b1, const void *w2,
                                   const float *b2, const void *w3, const float *b3, void *scratch, int64_t scratch_bytes,
                                   int32_t *sum_out, uint8_t *action_out, void *stream) {
    return launch_playout_cards_net(k_playout_net_deal_hidden, e, worlds, salt, seats, seats_per_game, (const u64 *)played, net_seats,
                                    TK_WEIGHTS(w1, b1, w2, b2, w3, b3), scratch, scratch_bytes, sum_out, action_out, stream, 0, 0.f);
}

int tarok_playout_cards_net_value(tarok_env *e, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game, int kind,
                                  const void *words, int net_seats, int depth, float value_scale, const void *w1, const float *b1,
                                  const void *w2, const float *b2, const void *w3, const float *b3, void *scratch, int64_t scratch_bytes,
                                  int32_t *sum_out, uint8_t *action_out, void *stream) {
    // DET with words is refused here; VOIDS / HIDDEN without them by the launcher, as the plain entries of those kinds
    if (!world_kind_ok(kind) || (kind == TAROK_NET_WORLDS_DET && words) || !depth_args_ok(depth, 1, TAROK_PLAYOUT_MAX_DEPTH, value_scale))
        return TAROK_EINVAL;
    return for_world_kind(kind, words, [&](auto k, auto *kwords) {
        const auto deal = TK_OF_KIND(k, k_playout_net_deal_value, k_playout_net_deal_value_voids, k_playout_net_deal_value_hidden);
        return launch_playout_cards_net(deal, e, worlds, salt, seats, seats_per_game, kwords, net_seats, TK_WEIGHTS(w1, b1, w2, b2, w3, b3),
                                        scratch, scratch_bytes, sum_out, action_out, stream, depth, value_scale);
    });
}

int tarok_playout_exchange(tarok_env *e, int worlds, int samples, int discard_sets, uint64_t salt, int seats,
                           const uint8_t *seats_per_game, int32_t *sum_out, int8_t *choice_out, uint8_t *discards_out, void *stream) {
    if (!playout_args_ok(e, worlds, samples, seats) || discard_sets < 1 || discard_sets > TAROK_EXCHANGE_MAX_SETS) return TAROK_EINVAL;
    if (!sum_out && !choice_out && !discards_out) return TAROK_OK;
    HIPCHK(hipSetDevice(e->device));
    // never fewer than 16 lanes per game: at most 16 teams per workgroup, whose 48 rows each are the 12 KiB the card launches use
    static_assert(TAROK_EXCHANGE_ROWS == TK_PX_ROWS && TAROK_EXCHANGE_MAX_SETS * 6 == TK_PX_ROWS, "6 groups x 8 sets");
    const u32 lg = playout_lg(TK_PX_MIN_LG, worlds * samples);
    hipLaunchKernelGGL(k_playout_exchange, playout_grid(e, lg), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed ^ (u64)salt, e->offset,
                       (u32)worlds, (u32)samples, (u32)discard_sets, lg, (u32)seats, seats_per_game, e->s01, e->s23, e->cnt, e->gkey,
                       reinterpret_cast<int4 *>(sum_out), choice_out, discards_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int64_t tarok_playout_exchange_net_scratch(const tarok_env *e, int worlds, int discard_sets) {
    if (!e || worlds < 1 || worlds > TAROK_PLAYOUT_MAX_WORLDS || discard_sets < 1 || discard_sets > TAROK_EXCHANGE_MAX_SETS) return TAROK_EINVAL;
    return e->n * 6 * (int64_t)discard_sets * (int64_t)worlds * TK_PN_ITEM_BYTES;
}

int tarok_playout_exchange_net(tarok_env *e, int worlds, int discard_sets, uint64_t salt, int seats, const uint8_t *seats_per_game,
                               int net_seats, const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                               const float *b3, void *scratch, int64_t scratch_bytes, int32_t *sum_out, int8_t *choice_out,
                               uint8_t *discards_out, void *stream) {
    return launch_playout_exchange_net(e, worlds, discard_sets, salt, seats, seats_per_game, net_seats, TK_WEIGHTS(w1, b1, w2, b2, w3, b3),
                                       scratch, scratch_bytes, sum_out, choice_out, discards_out, stream, 0, 0.f);
}

int tarok_playout_exchange_net_value(tarok_env *e, int worlds, int discard_sets, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                     int net_seats, int depth, float value_scale, const void *w1, const float *b1, const void *w2,
                                     const float *b2, const void *w3, const float *b3, void *scratch, int64_t scratch_bytes,
                                     int32_t *sum_out, int8_t *choice_out, uint8_t *discards_out, void *stream) {
    if (!depth_args_ok(depth, 1, TAROK_PLAYOUT_FRONT_MAX_DEPTH, value_scale)) return TAROK_EINVAL;
    return launch_playout_exchange_net(e, worlds, discard_sets, salt, seats, seats_per_game, net_seats, TK_WEIGHTS(w1, b1, w2, b2, w3, b3),
                                       scratch, scratch_bytes, sum_out, choice_out, discards_out, stream, depth, value_scale);
}

int tarok_shown_voids(tarok_env *e, uint32_t *voids_out, void *stream) {
    if (!e || !voids_out || !e->hist) return TAROK_EINVAL;              // needs a TAROK_HISTORY env
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_shown_voids, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->s01, e->s23, e->hist, voids_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_playout_cards_voids(tarok_env *e, int worlds, int samples, uint64_t salt, int seats, const uint8_t *seats_per_game,
                              const uint32_t *voids, int32_t *sum_out, uint8_t *action_out, void *stream) {
    return launch_playout_cards<true>(k_playout_voids, e, worlds, samples, salt, seats, seats_per_game, sum_out, action_out, stream, voids);
}

int tarok_played_cards(tarok_env *e, uint64_t *played_out, void *stream) {
    if (!e || !played_out || !e->hist) return TAROK_EINVAL;             // needs a TAROK_HISTORY env
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_played_cards, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->s01, e->s23, e->hist,
                       (u64 *)played_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_playout_cards_hidden(tarok_env *e, int worlds, int samples, uint64_t salt, int seats, const uint8_t *seats_per_game,
                               const uint64_t *played, int32_t *sum_out, uint8_t *action_out, void *stream) {
    return launch_playout_cards<true>(k_playout_hidden, e, worlds, samples, salt, seats, seats_per_game, sum_out, action_out, stream,
                                      (const u64 *)played);
}

int tarok_playout_cards_halving(tarok_env *e, int kind, const void *words, int rounds, const int *round_worlds, int samples, uint64_t salt,
                                int seats, const uint8_t *seats_per_game, int32_t *sum_out, int32_t *count_out, uint8_t *action_out,
                                void *stream) {
    if (!world_kind_ok(kind) || (kind == TAROK_NET_WORLDS_DET) != !words) return TAROK_EINVAL;
    return for_world_kind(kind, words, [&](auto k, auto *kwords) {
        return launch_playout_halving(TK_OF_KIND(k, k_playout_halving_det, k_playout_halving_voids, k_playout_halving_hidden), e, rounds,
                                      round_worlds, samples, salt, seats, seats_per_game, sum_out, count_out, action_out, stream, kwords);
    });
}

int64_t tarok_playout_net_halving_scratch_bytes(const tarok_env *e, int rounds, const int *round_worlds) {
    NetHalvingPlan p;
    return net_halving_plan(e, rounds, round_worlds, p) ? p.list.bytes : (int64_t)TAROK_EINVAL;
}

// tarok_playout_cards_net_halving, and — b non-NULL, the roles checked by the caller — tarok_playout_cards_net_versus_halving: the
// same rounds with launch_net_play's VERSUS form, whose items carry their viewers at every depth.
static int launch_playout_cards_net_halving(tarok_env *e, int kind, const void *words, int rounds, const int *round_worlds, uint64_t salt,
                                            int seats, const uint8_t *seats_per_game, int net_seats, const PolicyWeights &w, int depth,
                                            float value_scale, void *scratch, int64_t scratch_bytes, int32_t *sum_out, int32_t *count_out,
                                            uint8_t *action_out, void *stream, const PolicyWeights *b = nullptr, int own_rel = 0,
                                            int opp_rel = 0) {
    NetHalvingPlan p;
    // depth 0 is "to the last card", and a bad value_scale is refused there too
    if (!e || !world_kind_ok(kind) || (kind == TAROK_NET_WORLDS_DET) != !words || !net_halving_plan(e, rounds, round_worlds, p) ||
        seats < 0 || seats > 15 || !net_args_ok(net_seats, w, scratch, scratch_bytes, p.list.bytes) ||
        !depth_args_ok(depth, 0, TAROK_PLAYOUT_MAX_DEPTH, value_scale) || (!sum_out && !count_out && !action_out))
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    if (depth == TAROK_PLAYOUT_MAX_DEPTH) depth = 0;     // never stops: the plain kernels' bytes (§8.18)
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = e->n;
    const ListArrays a = p.list.carve(scratch);
    int4 *rsum = reinterpret_cast<int4 *>(a.extra);
    int *rcnt = reinterpret_cast<int *>(rsum + n * TAROK_PLAYOUT_RANKS);
    u32 *alive = a.on + n;
    const u64 pseed = e->seed ^ (u64)salt;
    const dim3 per_16((unsigned)((n + 15) / 16));
    hipLaunchKernelGGL(k_playout_net_list_init, per_16, dim3(TK_BLOCK), 0, s, n, (u32)seats, seats_per_game, e->s01, e->s23, a.on, alive,
                       rsum, reinterpret_cast<int4 *>(rcnt));
    return for_world_kind(kind, words, [&](auto k, auto *kwords) {
        const auto deal = depth || b ? TK_OF_KIND(k, k_playout_net_list_deal_value, k_playout_net_list_deal_value_voids,
                                                  k_playout_net_list_deal_value_hidden)
                                     : TK_OF_KIND(k, k_playout_net_list_deal, k_playout_net_list_deal_voids, k_playout_net_list_deal_hidden);
        for (int r = 0; r < p.h.rounds; r++) {
            const int wr = p.h.w[r];
            launch_list_scan(p.list, a, wr, s);
            const u32 lg = playout_lg(TK_PO_MIN_LG, wr);
            hipLaunchKernelGGL(deal, playout_grid(e, lg), dim3(TK_BLOCK), 0, s, n, pseed, e->offset, (u32)(p.h.end[r] - wr), (u32)wr, lg,
                               (u32)seats, seats_per_game, e->s01, e->s23, e->cnt, kwords, a.on, a.base, a.i01, a.i23, a.ikey, a.ires);
            launch_net_play(net_list_bound(n, (u32)r, (u32)wr), a.total, net_seats, a, w, s, depth, value_scale, b, own_rel, opp_rel);
            hipLaunchKernelGGL(k_playout_net_list_sum, per_16, dim3(TK_BLOCK), 0, s, n, (u32)p.h.end[r], (u32)wr,
                               (u32)(r == p.h.rounds - 1), (u32)seats, seats_per_game, e->s01, e->s23, e->gkey, a.ires, a.on, alive, a.base,
                               rsum, rcnt, reinterpret_cast<int4 *>(sum_out), reinterpret_cast<int4 *>(count_out), action_out);
        }
        HIPCHK(hipGetLastError());
        return (int)TAROK_OK;
    });
}

int tarok_playout_cards_net_halving(tarok_env *e, int kind, const void *words, int rounds, const int *round_worlds, uint64_t salt,
                                    int seats, const uint8_t *seats_per_game, int net_seats, const void *w1, const float *b1,
                                    const void *w2, const float *b2, const void *w3, const float *b3, int depth, float value_scale,
                                    void *scratch, int64_t scratch_bytes, int32_t *sum_out, int32_t *count_out, uint8_t *action_out,
                                    void *stream) {
    return launch_playout_cards_net_halving(e, kind, words, rounds, round_worlds, salt, seats, seats_per_game, net_seats,
                                            TK_WEIGHTS(w1, b1, w2, b2, w3, b3), depth, value_scale, scratch, scratch_bytes, sum_out,
                                            count_out, action_out, stream);
}

// The two versus entries' own refusals: the role sets, and network B where a seat plays it.  B may be absent when opp_rel = 0:
// the kernels then get A in its place, and read neither.
static bool versus_args_ok(int own_rel, int opp_rel, const PolicyWeights &a, PolicyWeights &b) {
    if (!net_versus_roles_ok(own_rel, opp_rel)) return false;
    if (!opp_rel) b = a;
    return b.w1 && b.b1 && b.w2 && b.b2 && b.w3 && b.b3;
}

int tarok_playout_cards_net_versus(tarok_env *e, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game, int kind,
                                   const void *words, int own_rel, int opp_rel, int depth, float value_scale, const void *w1,
                                   const float *b1, const void *w2, const float *b2, const void *w3, const float *b3, const void *v1,
                                   const float *c1, const void *v2, const float *c2, const void *v3, const float *c3, void *scratch,
                                   int64_t scratch_bytes, int32_t *sum_out, uint8_t *action_out, void *stream) {
    const PolicyWeights a = TK_WEIGHTS(w1, b1, w2, b2, w3, b3);
    PolicyWeights b = TK_WEIGHTS(v1, c1, v2, c2, v3, c3);
    // DET with words is refused here; VOIDS / HIDDEN without them by the launcher, as tarok_playout_cards_net_value
    if (!world_kind_ok(kind) || (kind == TAROK_NET_WORLDS_DET && words) || !depth_args_ok(depth, 0, TAROK_PLAYOUT_MAX_DEPTH, value_scale) ||
        !versus_args_ok(own_rel, opp_rel, a, b))
        return TAROK_EINVAL;
    if (depth == TAROK_PLAYOUT_MAX_DEPTH) depth = 0;     // never stops (§8.18)
    return for_world_kind(kind, words, [&](auto k, auto *kwords) {
        const auto deal = TK_OF_KIND(k, k_playout_net_deal_value, k_playout_net_deal_value_voids, k_playout_net_deal_value_hidden);
        return launch_playout_cards_net(deal, e, worlds, salt, seats, seats_per_game, kwords, 0, a, scratch, scratch_bytes, sum_out,
                                        action_out, stream, depth, value_scale, &b, own_rel, opp_rel);
    });
}

int64_t tarok_playout_cards_net_sampled_scratch(const tarok_env *e, int worlds, int samples) {
    if (!e || worlds < 1 || worlds > TAROK_PLAYOUT_MAX_WORLDS || samples < 1 || samples > TAROK_PLAYOUT_MAX_SAMPLES) return TAROK_EINVAL;
    const int64_t items = net_sampled_items(e->n, (u32)worlds, (u32)samples);
    return items < 0 ? (int64_t)TAROK_EINVAL : items * TK_PN_ITEM_BYTES;
}

// tarok_set_play_mode's checks and its conversion, for a mode that is an argument and not the env's.
static bool play_mode_of(float temperature, float epsilon, PlayMode &pm) {
    if (temperature != temperature || epsilon != epsilon) return false;
    if (!(epsilon >= 0.f && epsilon <= 1.f)) return false;
    if (temperature < 0.f || (temperature > 0.f && temperature < 1e-6f) || temperature > 1e6f) return false;
    pm.greedy = temperature == 0.f;
    pm.inv_t = pm.greedy ? 1.f : 1.0f / temperature;
    pm.thr = (uint32_t)floor((double)epsilon * 16777216.0);
    pm.eps = (float)pm.thr * (1.0f / 16777216.0f);
    return true;
}

int tarok_playout_cards_net_sampled(tarok_env *e, int worlds, int samples, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                    int kind, const void *words, int own_rel, int opp_rel, int depth, float value_scale,
                                    float temperature_a, float epsilon_a, float temperature_b, float epsilon_b, const void *w1,
                                    const float *b1, const void *w2, const float *b2, const void *w3, const float *b3, const void *v1,
                                    const float *c1, const void *v2, const float *c2, const void *v3, const float *c3, void *scratch,
                                    int64_t scratch_bytes, int32_t *sum_out, uint8_t *action_out, void *stream) {
    const PolicyWeights a = TK_WEIGHTS(w1, b1, w2, b2, w3, b3);
    PolicyWeights b = TK_WEIGHTS(v1, c1, v2, c2, v3, c3);
    PlayMode modes[2];
    // (the scratch function refuses samples out of range and a count that reaches 2^31 items: the launcher's need is then < 0)
    if (!world_kind_ok(kind) || (kind == TAROK_NET_WORLDS_DET && words) || !depth_args_ok(depth, 0, TAROK_PLAYOUT_MAX_DEPTH, value_scale) ||
        !versus_args_ok(own_rel, opp_rel, a, b) || !play_mode_of(temperature_a, epsilon_a, modes[0]) ||
        !play_mode_of(temperature_b, epsilon_b, modes[1]))
        return TAROK_EINVAL;
    if (depth == TAROK_PLAYOUT_MAX_DEPTH) depth = 0;     // never stops (§8.18)
    return for_world_kind(kind, words, [&](auto k, auto *kwords) {
        const auto deal = TK_OF_KIND(k, k_playout_net_deal_sampled, k_playout_net_deal_sampled_voids, k_playout_net_deal_sampled_hidden);
        return launch_playout_cards_net<true>(deal, e, worlds, salt, seats, seats_per_game, kwords, 0, a, scratch, scratch_bytes, sum_out,
                                              action_out, stream, depth, value_scale, &b, own_rel, opp_rel, samples, modes);
    });
}

int tarok_playout_cards_net_versus_halving(tarok_env *e, int kind, const void *words, int rounds, const int *round_worlds, uint64_t salt,
                                           int seats, const uint8_t *seats_per_game, int own_rel, int opp_rel, const void *w1,
                                           const float *b1, const void *w2, const float *b2, const void *w3, const float *b3,
                                           const void *v1, const float *c1, const void *v2, const float *c2, const void *v3,
                                           const float *c3, int depth, float value_scale, void *scratch, int64_t scratch_bytes,
                                           int32_t *sum_out, int32_t *count_out, uint8_t *action_out, void *stream) {
    const PolicyWeights a = TK_WEIGHTS(w1, b1, w2, b2, w3, b3);
    PolicyWeights b = TK_WEIGHTS(v1, c1, v2, c2, v3, c3);
    if (!versus_args_ok(own_rel, opp_rel, a, b)) return TAROK_EINVAL;
    return launch_playout_cards_net_halving(e, kind, words, rounds, round_worlds, salt, seats, seats_per_game, 0, a, depth, value_scale,
                                            scratch, scratch_bytes, sum_out, count_out, action_out, stream, &b, own_rel, opp_rel);
}

int tarok_playout_bids(tarok_env *e, uint32_t episode, const uint8_t *deals, int worlds, int samples, int contracts, uint64_t salt,
                       int seats, const uint8_t *seats_per_game, int32_t *sum_out, void *stream) {
    return launch_playout_bids(k_playout_bids, e, episode, deals, worlds, samples, contracts, salt, seats, seats_per_game, sum_out, stream);
}

int tarok_playout_bids_pass(tarok_env *e, uint32_t episode, const uint8_t *deals, int worlds, int samples, int contracts, uint64_t salt,
                            int seats, const uint8_t *seats_per_game, int32_t *sum_out, void *stream) {
    return launch_playout_bids(k_playout_bids_pass, e, episode, deals, worlds, samples, contracts, salt, seats, seats_per_game, sum_out, stream);
}

// the items, then k_bid_deal's 40 bytes per game: the launch allocates nothing, the env's own bidding buffer is not used
int64_t tarok_playout_bids_net_scratch(const tarok_env *e, int worlds) {
    if (!e || worlds < 1 || worlds > TAROK_PLAYOUT_MAX_WORLDS) return TAROK_EINVAL;
    return e->n * 4 * TAROK_BID_ROWS * (int64_t)worlds * TK_PN_ITEM_BYTES + e->n * 5 * (int64_t)sizeof(u64);
}

int tarok_playout_bids_net(tarok_env *e, uint32_t episode, const uint8_t *deals, int worlds, int contracts, uint64_t salt, int seats,
                           const uint8_t *seats_per_game, int net_seats, const void *w1, const float *b1, const void *w2, const float *b2,
                           const void *w3, const float *b3, void *scratch, int64_t scratch_bytes, int32_t *sum_out, void *stream) {
    return launch_playout_bids_net(e, episode, deals, worlds, contracts, salt, seats, seats_per_game, net_seats,
                                   TK_WEIGHTS(w1, b1, w2, b2, w3, b3), scratch, scratch_bytes, sum_out, stream, 0, 0.f, 0);
}

int tarok_playout_bids_net_value(tarok_env *e, uint32_t episode, const uint8_t *deals, int worlds, int contracts, uint64_t salt, int seats,
                                 const uint8_t *seats_per_game, int net_seats, int depth, float value_scale, int pass_value, const void *w1,
                                 const float *b1, const void *w2, const float *b2, const void *w3, const float *b3, void *scratch,
                                 int64_t scratch_bytes, int32_t *sum_out, void *stream) {
    if (!depth_args_ok(depth, 1, TAROK_PLAYOUT_FRONT_MAX_DEPTH, value_scale) || pass_value < 0 || pass_value > 1) return TAROK_EINVAL;
    return launch_playout_bids_net(e, episode, deals, worlds, contracts, salt, seats, seats_per_game, net_seats,
                                   TK_WEIGHTS(w1, b1, w2, b2, w3, b3), scratch, scratch_bytes, sum_out, stream, depth, value_scale, pass_value);
}

int64_t tarok_playout_exchange_net_list_scratch(const tarok_env *e, int worlds, int discard_sets) {
    ListScratch p;
    return exchange_list_plan(e, worlds, discard_sets, p) ? p.bytes : (int64_t)TAROK_EINVAL;
}

// tarok_playout_exchange_net / _value on the compacted list: the on words, the scan, the items, the playouts, the sums and the
// choice — seven launches on `stream`, nothing allocated, no host read.
int tarok_playout_exchange_net_list(tarok_env *e, int worlds, int discard_sets, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                    int net_seats, int depth, float value_scale, const void *w1, const float *b1, const void *w2,
                                    const float *b2, const void *w3, const float *b3, void *scratch, int64_t scratch_bytes,
                                    int32_t *sum_out, int8_t *choice_out, uint8_t *discards_out, void *stream) {
    ListScratch p;
    const PolicyWeights w = TK_WEIGHTS(w1, b1, w2, b2, w3, b3);
    // depth 0 is "to the last card", and a bad value_scale is refused there too
    if (!playout_args_ok(e, worlds, 1, seats) || !exchange_list_plan(e, worlds, discard_sets, p) ||
        !depth_args_ok(depth, 0, TAROK_PLAYOUT_FRONT_MAX_DEPTH, value_scale) || !net_args_ok(net_seats, w, scratch, scratch_bytes, p.bytes) ||
        (!sum_out && !choice_out && !discards_out))
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const ListArrays a = p.carve(scratch);
    const u64 pseed = e->seed ^ (u64)salt;
    hipLaunchKernelGGL(k_playout_exchange_net_list_init, grid_for(p.units), dim3(TK_BLOCK), 0, s, p.units, (u32)discard_sets, (u32)seats,
                       seats_per_game, e->s01, e->s23, a.on);
    launch_list_scan(p, a, worlds, s);
    launch_exchange_list_deal(e, a, p.bound, pseed, 0, worlds, discard_sets, seats, seats_per_game, depth, s);
    launch_net_play(p.bound, a.total, net_seats, a, w, s, depth, value_scale);
    hipLaunchKernelGGL(k_playout_exchange_net_list_sum, dim3((unsigned)((e->n + 15) / 16)), dim3(TK_BLOCK), 0, s, e->n, (u32)p.bound, pseed,
                       e->offset, (u32)worlds, (u32)discard_sets, (u32)seats, seats_per_game, e->s01, e->s23, e->cnt, e->gkey, a.on, a.base,
                       a.ires, reinterpret_cast<int4 *>(sum_out), choice_out, discards_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int64_t tarok_playout_bids_net_list_scratch(const tarok_env *e, int worlds, int contracts, int seats, int per_game_seats, int pass_value) {
    ListScratch p;
    return bid_list_plan(e, worlds, contracts, seats, per_game_seats, pass_value, p) ? p.bytes : (int64_t)TAROK_EINVAL;
}

// tarok_playout_bids_net / _value on the compacted list: the deal, the on words, the scan, the items, the playouts, the sums —
// eight launches on `stream`, nothing allocated, no host read.  pass_value with depth 0: the _value launch at the depth that
// never stops, which is the only launch that values a pass.
int tarok_playout_bids_net_list(tarok_env *e, uint32_t episode, const uint8_t *deals, int worlds, int contracts, uint64_t salt, int seats,
                                const uint8_t *seats_per_game, int net_seats, int depth, float value_scale, int pass_value, const void *w1,
                                const float *b1, const void *w2, const float *b2, const void *w3, const float *b3, void *scratch,
                                int64_t scratch_bytes, int32_t *sum_out, void *stream) {
    ListScratch p;
    const PolicyWeights w = TK_WEIGHTS(w1, b1, w2, b2, w3, b3);
    // depth 0 is "to the last card", and a bad value_scale is refused there too
    if (!playout_args_ok(e, worlds, 1, seats) || !bid_list_plan(e, worlds, contracts, seats, seats_per_game != nullptr, pass_value, p) ||
        !depth_args_ok(depth, 0, TAROK_PLAYOUT_FRONT_MAX_DEPTH, value_scale) || !net_args_ok(net_seats, w, scratch, scratch_bytes, p.bytes) ||
        !sum_out)
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    if (pass_value && !depth) depth = TAROK_PLAYOUT_FRONT_MAX_DEPTH;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = e->n, rows = n * 4 * TAROK_BID_ROWS;
    const ListArrays a = p.carve(scratch);
    u64 *deal = reinterpret_cast<u64 *>(a.extra);
    hipLaunchKernelGGL(k_bid_deal, grid_for(n), dim3(TK_BLOCK), 0, s, n, e->seed, e->offset, episode, deals, deal);
    hipLaunchKernelGGL(k_playout_bids_net_list_init, grid_for(p.units), dim3(TK_BLOCK), 0, s, n, (u32)contracts, (u32)pass_value, (u32)seats,
                       seats_per_game, deal, a.on);
    launch_list_scan(p, a, worlds, s);
    launch_bids_list_deal(e, a, p.bound, e->seed ^ (u64)salt, episode, 0, worlds, seats, seats_per_game, deal, depth, pass_value, s);
    launch_net_play(p.bound, a.total, net_seats, a, w, s, depth, value_scale);
    hipLaunchKernelGGL(k_playout_bids_net_list_sum, grid_for(rows), dim3(TK_BLOCK), 0, s, rows, (u32)p.bound, (u32)worlds, a.on, a.base,
                       a.ires, sum_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int64_t tarok_playout_exchange_net_halving_scratch_bytes(const tarok_env *e, int rounds, const int *round_worlds, int discard_sets) {
    FrontHalvingPlan p;
    return exchange_halving_plan(e, rounds, round_worlds, discard_sets, p) ? p.list.bytes : (int64_t)TAROK_EINVAL;
}

// tarok_playout_exchange_net_list with sequential halving over a game's candidates: the init, then per round the scan, the
// round's items, the playouts and the sums with the survivor rule — 1 + 6 x rounds launches on `stream`, nothing allocated, no
// host read.
int tarok_playout_exchange_net_halving(tarok_env *e, int rounds, const int *round_worlds, int discard_sets, uint64_t salt, int seats,
                                       const uint8_t *seats_per_game, int net_seats, int depth, float value_scale, const void *w1,
                                       const float *b1, const void *w2, const float *b2, const void *w3, const float *b3, void *scratch,
                                       int64_t scratch_bytes, int32_t *sum_out, int32_t *count_out, int8_t *choice_out,
                                       uint8_t *discards_out, void *stream) {
    FrontHalvingPlan p;
    const PolicyWeights w = TK_WEIGHTS(w1, b1, w2, b2, w3, b3);
    // depth 0 is "to the last card", and a bad value_scale is refused there too
    if (!e || seats < 0 || seats > 15 || !exchange_halving_plan(e, rounds, round_worlds, discard_sets, p) ||
        !depth_args_ok(depth, 0, TAROK_PLAYOUT_FRONT_MAX_DEPTH, value_scale) ||
        !net_args_ok(net_seats, w, scratch, scratch_bytes, p.list.bytes) || (!sum_out && !count_out && !choice_out && !discards_out))
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = e->n;
    const ListArrays a = p.list.carve(scratch);
    int4 *rsum = reinterpret_cast<int4 *>(a.extra);
    int *rcnt = reinterpret_cast<int *>(rsum + n * 6 * discard_sets);
    u32 *alive = a.on + p.list.units;
    const u64 pseed = e->seed ^ (u64)salt;
    hipLaunchKernelGGL(k_playout_exchange_net_halving_init, grid_for(p.list.units), dim3(TK_BLOCK), 0, s, p.list.units, (u32)discard_sets,
                       (u32)seats, seats_per_game, e->s01, e->s23, a.on, alive, rsum, rcnt);
    for (int r = 0; r < p.h.rounds; r++) {
        const int wr = p.h.w[r];
        const u32 bound = (u32)p.round_bound[r];
        launch_list_scan(p.list, a, wr, s);
        launch_exchange_list_deal(e, a, p.round_bound[r], pseed, p.h.end[r] - wr, wr, discard_sets, seats, seats_per_game, depth, s);
        launch_net_play(p.round_bound[r], a.total, net_seats, a, w, s, depth, value_scale);
        hipLaunchKernelGGL(k_playout_exchange_net_halving_sum, dim3((unsigned)((n + 15) / 16)), dim3(TK_BLOCK), 0, s, n, bound, pseed,
                           e->offset, (u32)p.h.end[r], (u32)wr, (u32)(r == p.h.rounds - 1), (u32)discard_sets, (u32)seats, seats_per_game,
                           e->s01, e->s23, e->cnt, e->gkey, a.ires, a.on, alive, a.base, rsum, rcnt, reinterpret_cast<int4 *>(sum_out),
                           count_out, choice_out, discards_out);
    }
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int64_t tarok_playout_bids_net_halving_scratch_bytes(const tarok_env *e, int rounds, const int *round_worlds, int contracts, int seats,
                                                     int per_game_seats, int pass_value) {
    FrontHalvingPlan p;
    return bid_halving_plan(e, rounds, round_worlds, contracts, seats, per_game_seats, pass_value, p) ? p.list.bytes : (int64_t)TAROK_EINVAL;
}

// tarok_playout_bids_net_list with sequential halving over a unit's rows: the deal, the init, then per round the scan, the
// round's items, the playouts and the sums with the survivor rule — 2 + 6 x rounds launches on `stream`, nothing allocated, no
// host read.  pass_value with depth 0: the _value kernels at the depth that never stops, as the list launch.
int tarok_playout_bids_net_halving(tarok_env *e, uint32_t episode, const uint8_t *deals, int rounds, const int *round_worlds, int contracts,
                                   uint64_t salt, int seats, const uint8_t *seats_per_game, int net_seats, int depth, float value_scale,
                                   int pass_value, const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                                   const float *b3, void *scratch, int64_t scratch_bytes, int32_t *sum_out, int32_t *count_out,
                                   int32_t *value_out, void *stream) {
    FrontHalvingPlan p;
    const PolicyWeights w = TK_WEIGHTS(w1, b1, w2, b2, w3, b3);
    if (!e || !bid_halving_plan(e, rounds, round_worlds, contracts, seats, seats_per_game != nullptr, pass_value, p) ||
        !depth_args_ok(depth, 0, TAROK_PLAYOUT_FRONT_MAX_DEPTH, value_scale) ||
        !net_args_ok(net_seats, w, scratch, scratch_bytes, p.list.bytes) || (!sum_out && !count_out && !value_out))
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    if (pass_value && !depth) depth = TAROK_PLAYOUT_FRONT_MAX_DEPTH;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = e->n;
    const ListArrays a = p.list.carve(scratch);
    int *rsum = reinterpret_cast<int *>(a.extra);
    int *rcnt = rsum + n * 4 * TAROK_BID_ROWS;
    u64 *deal = reinterpret_cast<u64 *>(rcnt + n * 4 * TAROK_BID_ROWS);
    u32 *alive = a.on + p.list.units;
    hipLaunchKernelGGL(k_bid_deal, grid_for(n), dim3(TK_BLOCK), 0, s, n, e->seed, e->offset, episode, deals, deal);
    hipLaunchKernelGGL(k_playout_bids_net_halving_init, grid_for(p.list.units), dim3(TK_BLOCK), 0, s, n, (u32)contracts, (u32)pass_value,
                       (u32)seats, seats_per_game, deal, a.on, alive, reinterpret_cast<int4 *>(rsum), reinterpret_cast<int4 *>(rcnt));
    for (int r = 0; r < p.h.rounds; r++) {
        const int wr = p.h.w[r];
        const u32 bound = (u32)p.round_bound[r];
        launch_list_scan(p.list, a, wr, s);
        launch_bids_list_deal(e, a, p.round_bound[r], e->seed ^ (u64)salt, episode, p.h.end[r] - wr, wr, seats, seats_per_game, deal, depth,
                              pass_value, s);
        launch_net_play(p.round_bound[r], a.total, net_seats, a, w, s, depth, value_scale);
        hipLaunchKernelGGL(k_playout_bids_net_halving_sum, dim3((unsigned)((p.list.units + 7) / 8)), dim3(TK_BLOCK), 0, s, p.list.units,
                           bound, (u32)p.h.end[r], (u32)wr, (u32)(r == p.h.rounds - 1), (u32)p.h.worlds, a.ires, a.on, alive, a.base, rsum,
                           rcnt, sum_out, count_out, value_out);
    }
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

extern "C++" {
template <class Kernel>
static int launch_bid_round(Kernel kernel, tarok_env *e, uint32_t episode, const int32_t *sums, int playouts, int threshold, int contracts,
                            int seats, const uint8_t *seats_per_game, int8_t *contract_out, int8_t *declarer_out, int8_t *king_out,
                            void *stream) {
    if (!e || playouts < 1 || contracts < 1 || contracts > TAROK_BID_ALL_CONTRACTS || seats < 0 || seats > 15 ||
        (!sums && (seats != 0 || seats_per_game)) || (!contract_out && !declarer_out && !king_out))
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(kernel, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed, e->offset, episode, sums, playouts,
                       threshold, (u32)contracts, (u32)(sums ? seats : 0), sums ? seats_per_game : nullptr, contract_out, declarer_out,
                       king_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}
}

int tarok_bid_round(tarok_env *e, uint32_t episode, const int32_t *sums, int playouts, int threshold, int contracts, int seats,
                    const uint8_t *seats_per_game, int8_t *contract_out, int8_t *declarer_out, int8_t *king_out, void *stream) {
    return launch_bid_round(k_bid_round, e, episode, sums, playouts, threshold, contracts, seats, seats_per_game, contract_out, declarer_out,
                            king_out, stream);
}

int tarok_bid_round_pass(tarok_env *e, uint32_t episode, const int32_t *sums, int playouts, int margin, int contracts, int seats,
                         const uint8_t *seats_per_game, int8_t *contract_out, int8_t *declarer_out, int8_t *king_out, void *stream) {
    return launch_bid_round(k_bid_round_pass, e, episode, sums, playouts, margin, contracts, seats, seats_per_game, contract_out,
                            declarer_out, king_out, stream);
}

extern "C++" {
template <class Kernel>
static int launch_bid_values(Kernel kernel, tarok_env *e, uint32_t episode, const uint8_t *deals, const void *w1, const float *b1,
                             const void *w2, const float *b2, const void *w3, const float *b3, float scale, int contracts, int seats,
                             const uint8_t *seats_per_game, int32_t *value_out, float *raw_out, uint64_t *feature_words_out, void *stream) {
    if (!e || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !(scale > 0.f) || scale > 1048576.f || contracts < 1 ||
        contracts > TAROK_BID_ALL_CONTRACTS || seats < 0 || seats > 15 || (!value_out && !raw_out && !feature_words_out))
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    if (!e->bid_deal) HIPCHK(hipMalloc((void **)&e->bid_deal, (size_t)e->n * 5 * sizeof(u64)));   // tarok_playout_bids' buffer
    hipLaunchKernelGGL(k_bid_deal, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed, e->offset, episode, deals, e->bid_deal);
    const int64_t games = PM_M / 4;                  // per workgroup: one 128-row tile
    hipLaunchKernelGGL(kernel, dim3((unsigned)((e->n + games - 1) / games)), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n,
                       e->bid_deal, (const __bf16 *)w1, b1, (const __bf16 *)w2, b2, (const __bf16 *)w3, b3, scale, (u32)contracts,
                       (u32)seats, seats_per_game, reinterpret_cast<int4 *>(value_out), reinterpret_cast<float4 *>(raw_out),
                       reinterpret_cast<ulonglong2 *>(feature_words_out));
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}
}

int tarok_bid_values(tarok_env *e, uint32_t episode, const uint8_t *deals, const void *w1, const float *b1, const void *w2,
                     const float *b2, const void *w3, const float *b3, float scale, int contracts, int seats,
                     const uint8_t *seats_per_game, int32_t *value_out, float *raw_out, uint64_t *feature_words_out, void *stream) {
    return launch_bid_values(k_bid_values, e, episode, deals, w1, b1, w2, b2, w3, b3, scale, contracts, seats, seats_per_game, value_out,
                             raw_out, feature_words_out, stream);
}

int tarok_bid_values_pass(tarok_env *e, uint32_t episode, const uint8_t *deals, const void *w1, const float *b1, const void *w2,
                          const float *b2, const void *w3, const float *b3, float scale, int contracts, int seats,
                          const uint8_t *seats_per_game, int32_t *value_out, float *raw_out, uint64_t *feature_words_out, void *stream) {
    return launch_bid_values(k_bid_values_pass, e, episode, deals, w1, b1, w2, b2, w3, b3, scale, contracts, seats, seats_per_game,
                             value_out, raw_out, feature_words_out, stream);
}

int tarok_exchange_values(tarok_env *e, const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                          const float *b3, int seats, const uint8_t *seats_per_game, float *raw_out, int8_t *choice_out,
                          uint8_t *discards_out, uint64_t *feature_words_out, void *stream) {
    if (!e || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || seats < 0 || seats > 15) return TAROK_EINVAL;
    if (!raw_out && !choice_out && !discards_out && !feature_words_out) return TAROK_OK;
    HIPCHK(hipSetDevice(e->device));
    const int64_t games = PM_M / 8;                  // per workgroup: one 128-row tile, eight rows a game
    hipLaunchKernelGGL(k_exchange_values, dim3((unsigned)((e->n + games - 1) / games)), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n,
                       e->s01, e->s23, e->gkey, (const __bf16 *)w1, b1, (const __bf16 *)w2, b2, (const __bf16 *)w3, b3, (u32)seats,
                       seats_per_game, reinterpret_cast<float4 *>(raw_out), choice_out, discards_out,
                       reinterpret_cast<ulonglong2 *>(feature_words_out));
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_exchange_candidates(tarok_env *e, int discard_sets, uint64_t salt, int seats, const uint8_t *seats_per_game,
                              uint8_t *cand_out, void *stream) {
    if (!e || discard_sets < 1 || discard_sets > TAROK_EXCHANGE_MAX_SETS || seats < 0 || seats > 15) return TAROK_EINVAL;
    if (!cand_out) return TAROK_OK;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_exchange_candidates, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed ^ (u64)salt, e->offset,
                       (u32)discard_sets, (u32)seats, seats_per_game, e->s01, e->s23, e->cnt, cand_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int64_t tarok_front_lines_scratch_bytes(int64_t n_games) {
    if (n_games <= 0 || n_games > (1LL << 31)) return TAROK_EINVAL;
    return TK_FRONT_HEAD_BYTES + n_games * TK_AHEAD * (int64_t)sizeof(u64);
}

int tarok_front_lines(tarok_env *e, const void *bw1, const float *bb1, const void *bw2, const float *bb2, const void *bw3,
                      const float *bb3, float scale, int playouts, int margin, int contracts, int pass_value, const void *xw1,
                      const float *xb1, const void *xw2, const float *xb2, const void *xw3, const float *xb3, int seats,
                      const uint8_t *seats_per_game, void *scratch, int64_t scratch_bytes, int64_t *count_out,
                      int64_t *contract_hist_out, void *stream) {
    if (!e) return TAROK_EINVAL;
    const int nb = !!bw1 + !!bb1 + !!bw2 + !!bb2 + !!bw3 + !!bb3, nx = !!xw1 + !!xb1 + !!xw2 + !!xb2 + !!xw3 + !!xb3;
    if ((nb != 0 && nb != 6) || (nx != 0 && nx != 6) || nb + nx == 0) return TAROK_EINVAL;
    if (nb && (!(scale > 0.f) || scale > 1048576.f || playouts < 1 || contracts < 1 || contracts > TAROK_BID_ALL_CONTRACTS ||
               e->mix != TAROK_MIX_BOT))
        return TAROK_EINVAL;
    if (seats < 0 || seats > 15 || !scratch || scratch_bytes < tarok_front_lines_scratch_bytes(e->n)) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *count = reinterpret_cast<unsigned long long *>(scratch);
    u64 *items = reinterpret_cast<u64 *>((char *)scratch + TK_FRONT_HEAD_BYTES);
    const int64_t cap = e->n * TK_AHEAD;
    hipLaunchKernelGGL(k_front_zero, dim3(1), dim3(64), 0, s, count, reinterpret_cast<unsigned long long *>(contract_hist_out));
    hipLaunchKernelGGL(k_front_select, grid_for(e->n), dim3(TK_BLOCK), 0, s, e->n, e->aux, e->cnt, count, items, cap);
    if (nb) {
        const dim3 grid((unsigned)((cap + PM_M / 4 - 1) / (PM_M / 4)));
#define TK_LAUNCH_FRONT_BID(P)                                                                                                \
        hipLaunchKernelGGL(k_front_bid<P>, grid, dim3(TK_BLOCK), 0, s, e->n, e->aux, count, items, (const __bf16 *)bw1, bb1,       \
                           (const __bf16 *)bw2, bb2, (const __bf16 *)bw3, bb3, scale, playouts, margin, (u32)contracts, (u32)seats, \
                           seats_per_game, nx ? 1 : 0)
        if (pass_value) TK_LAUNCH_FRONT_BID(true); else TK_LAUNCH_FRONT_BID(false);
#undef TK_LAUNCH_FRONT_BID
    }
    if (nx) {
        const dim3 grid((unsigned)((cap + PM_M / 8 - 1) / (PM_M / 8)));
#define TK_LAUNCH_FRONT_EXCHANGE(F)                                                                                           \
        hipLaunchKernelGGL(k_front_exchange<F>, grid, dim3(TK_BLOCK), 0, s, e->n, e->mix, e->aux, count, items, (const __bf16 *)xw1, \
                           xb1, (const __bf16 *)xw2, xb2, (const __bf16 *)xw3, xb3, (u32)seats, seats_per_game)
        if (nb) TK_LAUNCH_FRONT_EXCHANGE(true); else TK_LAUNCH_FRONT_EXCHANGE(false);
#undef TK_LAUNCH_FRONT_EXCHANGE
    }
    hipLaunchKernelGGL(k_front_mark, dim3((unsigned)((cap + TK_BLOCK - 1) / TK_BLOCK)), dim3(TK_BLOCK), 0, s, e->n, e->aux, count, items,
                       count_out, reinterpret_cast<unsigned long long *>(contract_hist_out));
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_get_lines(tarok_env *e, uint64_t *lines_out, uint64_t *lanes_out, void *stream) {
    if (!e) return TAROK_EINVAL;
    if (!lines_out && !lanes_out) return TAROK_OK;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_get_lines, grid_for(e->n * TK_AHEAD), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->aux, (u64 *)lines_out,
                       (u64 *)lanes_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_playout_targets(tarok_env *e, const int32_t *sums, const uint64_t *obs, int playouts, float tau, int seats,
                          const uint8_t *seats_per_game, void *target_out, void *stream) {
    if (!e || !sums || !obs || !target_out || playouts < 1 || !(tau >= 0.f) || tau > 3.0e38f || seats < 0 || seats > 15) return TAROK_EINVAL;
    const float den = (float)playouts * tau;      // the kernel's divisor: a normal float32 number, or 0 with tau = 0
    if (tau > 0.f && !(den >= 1.17549435e-38f && den <= 3.0e38f)) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_playout_targets, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, reinterpret_cast<const int4 *>(sums),
                       (const u64 *)obs, den, (u32)seats, seats_per_game, reinterpret_cast<uint4 *>(target_out));
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_playout_targets_counts(tarok_env *e, const int32_t *sums, const int32_t *counts, const uint64_t *obs, float tau, int seats,
                                 const uint8_t *seats_per_game, void *target_out, void *stream) {
    if (!e || !sums || !counts || !obs || !target_out || !(tau >= 0.f) || tau > 3.0e38f || seats < 0 || seats > 15) return TAROK_EINVAL;
    if (tau > 0.f && tau < 1.17549435e-38f) return TAROK_EINVAL;      // the kernel's divisor: a normal float32 number, or 0
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_playout_targets_counts, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n,
                       reinterpret_cast<const int4 *>(sums), reinterpret_cast<const int4 *>(counts), (const u64 *)obs, tau, (u32)seats,
                       seats_per_game, reinterpret_cast<uint4 *>(target_out));
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_debug_stamps_sized(tarok_env *e, uint64_t *stamps, int64_t n_words) {
    if (!e || n_words < 0 || (stamps && n_words == 0)) return TAROK_EINVAL;
    e->stamps = (u64 *)stamps;
    e->stamps_words = stamps ? (size_t)n_words : 0;
    return TAROK_OK;      // (graphs captured with another stamps pointer stay cached under their own key)
}

int tarok_debug_stamps(tarok_env *e, uint64_t *stamps) {      // the step kernels' size: [ceil(N/64), 3]
    if (!e) return TAROK_EINVAL;
    return tarok_debug_stamps_sized(e, stamps, stamps ? 3 * ((e->n + 63) / 64) : 0);
}

int tarok_debug_refill_selftest(tarok_env *e, int kind, int per_slot, uint32_t episode0, int order, int reps, uint64_t *report_out) {
    if (!e || kind < 0 || kind > 3 || per_slot < 1 || per_slot > TK_AHEAD || order < 0 || order > 2 || reps < 1 || !report_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    const int64_t n = e->n;
    const size_t rows = 4;
    void *buf = nullptr;
    unsigned long long *rep = nullptr;
    HIPCHK(hipMalloc(&buf, rows * (size_t)n * (8 + 8 + 1 + 1) + 64));
    hipError_t r = hipMalloc((void **)&rep, 49 * sizeof(unsigned long long));
    if (r == hipSuccess) r = hipMemset(rep, 0, 49 * sizeof(unsigned long long));
    if (r != hipSuccess) { (void)hipFree(buf); g_last_hip = (int)r; return TAROK_EHIP; }
    uint64_t *obs = (uint64_t *)buf;
    int16_t *reward = (int16_t *)(obs + rows * n);
    uint8_t *action = (uint8_t *)(reward + rows * n * 4), *done = action + rows * n;
    u32 groups = (u32)((n + TK_BLOCK - 1) / TK_BLOCK);
    for (int it = 0; it < reps; it++) {
        hipLaunchKernelGGL(k_dbg_clear_lines, grid_for(n), dim3(TK_BLOCK), 0, 0, e->aux, n);
        hipLaunchKernelGGL(k_dbg_fill_lists, dim3(groups), dim3(TK_BLOCK), 0, 0, e->rlist, e->rcount, n, (u32)per_slot, episode0, (u32)order);
        if (kind == 0) launch_play(e, true, 1, n, nullptr, action, reward, done, nullptr, obs, TAROK_AUTO_RESET, 0);            // k_step, Bot policy
        else if (kind == 1) {                                                                                                  // k_step, cards given
            hipLaunchKernelGGL(k_legal, grid_for(n), dim3(TK_BLOCK), 0, 0, n, e->s01, e->s23, (u64 *)obs, (int8_t *)nullptr);
            launch_policy(e, obs, action, 0);
            launch_play(e, false, 1, n, action, nullptr, reward, done, nullptr, obs, TAROK_AUTO_RESET, 0);
        } else launch_play(e, true, kind == 2 ? 4 : 2, n, nullptr, action, reward, done, nullptr, obs, TAROK_AUTO_RESET, 0);    // k_play_wide
        hipLaunchKernelGGL(k_dbg_check_lines, grid_for(n), dim3(TK_BLOCK), 0, 0, e->aux, n, e->seed, e->offset, e->mix, (u32)per_slot, episode0, rep);
    }
    r = hipDeviceSynchronize();
    if (r == hipSuccess) r = hipMemcpy(report_out, rep, 49 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    // the lists and lines of the env are the test's now: empty them all and deal every slot's lines afresh
    if (r == hipSuccess) r = hipMemset(e->rcount, 0, TK_RC(groups, 0) * sizeof(u32));
    if (r == hipSuccess) {
        hipLaunchKernelGGL(k_dbg_clear_lines, grid_for(n), dim3(TK_BLOCK), 0, 0, e->aux, n);
        r = hipDeviceSynchronize();
    }
    (void)hipFree(buf); (void)hipFree(rep);
    if (r != hipSuccess) { g_last_hip = (int)r; return TAROK_EHIP; }
    return TAROK_OK;
}

int tarok_observe(tarok_env *e, void *features_out, void *stream) {
    if (!e || !features_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_observe, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->s01, e->s23,
                       (uint2 *)features_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_observe_ref(tarok_env *e, uint8_t *record_out, int32_t *meta_out, void *stream) {
    if (!e || !record_out) return TAROK_EINVAL;
    if (!e->hist) return TAROK_EINVAL;                                   // needs a TAROK_HISTORY env
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_observe_ref, dim3((unsigned)((e->n + OR_GAMES - 1) / OR_GAMES)), dim3(256), 0, (hipStream_t)stream, e->n,
                       e->s01, e->s23, e->hist, (uint4 *)record_out, (int4 *)meta_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_observe_exchange_ref(tarok_env *e, uint8_t *out, void *stream) {
    if (!e || !out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_observe_exchange_ref, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->s01, e->s23,
                       (uint2 *)out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_observe_hands_ref(tarok_env *e, uint8_t *out, void *stream) {
    if (!e || !out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_observe_hands_ref, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->s01, e->s23,
                       (uint2 *)out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_get_history(tarok_env *e, uint8_t *hist_out, void *stream) {
    if (!e || !hist_out || !e->hist) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(hist_out, e->hist, (size_t)e->n * 48, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TAROK_OK;
}

int tarok_set_history(tarok_env *e, const uint8_t *hist_in, void *stream) {
    if (!e || !hist_in || !e->hist) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->hist, hist_in, (size_t)e->n * 48, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TAROK_OK;
}

int tarok_sample_policy(tarok_env *e, const void *logits_bf16, const uint64_t *obs, uint8_t *action_out,
                        float *logp_out, void *stream) {
    if (!e || !logits_bf16 || !obs || !action_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    if (!e->mode_on)
        hipLaunchKernelGGL(k_sample, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, (const uint4 *)logits_bf16,
                           (const u64 *)obs, e->gkey, action_out, logp_out);
    else
        hipLaunchKernelGGL(k_sample_mode, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, (const uint4 *)logits_bf16,
                           (const u64 *)obs, e->gkey, action_out, logp_out, e->inv_t, e->greedy, e->explore_thr, e->eps_p);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_policy_mlp(tarok_env *e, const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                     const float *b3, const uint64_t *obs, uint8_t *action_out, float *logp_out, float *value_out,
                     void *features_out, uint64_t *feature_words_out, void *stream) {
    if (!e || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !obs || !action_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    dim3 grid((unsigned)((e->n + PM_M - 1) / PM_M));
    if (!e->mode_on)
        hipLaunchKernelGGL(k_policy_mlp, grid, dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->s01, e->s23, (const u64 *)obs,
                           e->gkey, (const __bf16 *)w1, b1, (const __bf16 *)w2, b2, (const __bf16 *)w3, b3, action_out, logp_out,
                           value_out, (uint4 *)features_out, (ulonglong2 *)feature_words_out, stamps_for(e, 8 * (size_t)grid.x));
    else
        hipLaunchKernelGGL(k_policy_mlp_mode, grid, dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->s01, e->s23, (const u64 *)obs,
                           e->gkey, (const __bf16 *)w1, b1, (const __bf16 *)w2, b2, (const __bf16 *)w3, b3, action_out, logp_out,
                           value_out, (uint4 *)features_out, (ulonglong2 *)feature_words_out, stamps_for(e, 8 * (size_t)grid.x),
                           e->inv_t, e->greedy, e->explore_thr, e->eps_p);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// The launch of the four policy-step kinds (0: k_policy_step, 1: k_policy_step_seats, 2: k_policy_step_versus,
// 3: k_policy_step_pool, whose `b` is the six stacked arrays of the pool), the arguments checked by the caller: one grid (the play groups, then their refill workgroups), one argument list.
static int launch_policy_step(tarok_env *e, int kind, u32 seats, const uint8_t *seat_sets, const PolicyWeights &a,
                              const PolicyWeights &b, const uint64_t *obs, uint8_t *action_out, float *logp_out, float *value_out,
                              uint64_t *feature_words_out, int16_t *reward_out, uint8_t *done_out, uint16_t *trick_out,
                              uint64_t *obs_out, int flags, void *stream, u32 pool_size = 0, const uint8_t *group_net = nullptr) {
    HIPCHK(hipSetDevice(e->device));
    u32 groups = (u32)((e->n + TK_BLOCK - 1) / TK_BLOCK);
    u32 fan = e->refill_fan;
    dim3 grid(groups + (groups + fan - 1) / fan);
    e->launched = 1;
#define TK_LAUNCH_POLICY_STEP(K, ...)                                                                                      \
    hipLaunchKernelGGL(K, grid, dim3(2 * TK_BLOCK), 0, (hipStream_t)stream, e->n, e->seed, e->offset, e->mix, flags, groups,  \
                       e->epoch, fan, (const u64 *)obs, a.w1, a.b1, a.w2, a.b2, a.w3, a.b3, action_out, logp_out, value_out,  \
                       (ulonglong2 *)feature_words_out, reward_out, done_out, trick_out, (u64 *)obs_out, e->hist, e->s01,     \
                       e->s23, e->aux, e->cnt, e->gkey, e->rlist, e->rcount, ##__VA_ARGS__)
    if (!e->mode_on) {                    // play mode (1, 0): the launches as they always were
        if (kind == 0) TK_LAUNCH_POLICY_STEP(k_policy_step);
        else if (kind == 1) TK_LAUNCH_POLICY_STEP(k_policy_step_seats, seats, seat_sets);
        else if (kind == 2) TK_LAUNCH_POLICY_STEP(k_policy_step_versus, seats, seat_sets, b.w1, b.b1, b.w2, b.b2, b.w3, b.b3);
        else TK_LAUNCH_POLICY_STEP(k_policy_step_pool, seats, seat_sets, pool_size, b.w1, b.b1, b.w2, b.b2, b.w3, b.b3, group_net);
    } else {
#define TK_MODE_VALUES e->inv_t, e->greedy, e->explore_thr, e->eps_p
        if (kind == 0) TK_LAUNCH_POLICY_STEP(k_policy_step_mode, TK_MODE_VALUES);
        else if (kind == 1) TK_LAUNCH_POLICY_STEP(k_policy_step_seats_mode, seats, seat_sets, TK_MODE_VALUES);
        else if (kind == 2) TK_LAUNCH_POLICY_STEP(k_policy_step_versus_mode, seats, seat_sets, b.w1, b.b1, b.w2, b.b2, b.w3, b.b3, TK_MODE_VALUES);
        else TK_LAUNCH_POLICY_STEP(k_policy_step_pool_mode, seats, seat_sets, pool_size, b.w1, b.b1, b.w2, b.b2, b.w3, b.b3, group_net,
                                   TK_MODE_VALUES);
#undef TK_MODE_VALUES
    }
#undef TK_LAUNCH_POLICY_STEP
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_policy_step(tarok_env *e, const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                      const float *b3, const uint64_t *obs, uint8_t *action_out, float *logp_out, float *value_out,
                      uint64_t *feature_words_out, int16_t *reward_out, uint8_t *done_out, uint16_t *trick_out,
                      uint64_t *obs_out, int flags, void *stream) {
    if (!e || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !obs || !action_out || !obs_out) return TAROK_EINVAL;
    return launch_policy_step(e, 0, 15, nullptr, TK_WEIGHTS(w1, b1, w2, b2, w3, b3), PolicyWeights{}, obs, action_out, logp_out, value_out,
                              feature_words_out, reward_out, done_out, trick_out, obs_out, flags, stream);
}

int tarok_policy_step_seats(tarok_env *e, int seats, const uint8_t *seats_per_game, const void *w1, const float *b1, const void *w2,
                            const float *b2, const void *w3, const float *b3, const uint64_t *obs, uint8_t *action_out, float *logp_out,
                            float *value_out, uint64_t *feature_words_out, int16_t *reward_out, uint8_t *done_out, uint16_t *trick_out,
                            uint64_t *obs_out, int flags, void *stream) {
    if (!e || seats < 0 || seats > 15) return TAROK_EINVAL;       // (before the env is looked at, before any HIP call)
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !obs || !action_out || !obs_out || obs == obs_out) return TAROK_EINVAL;
    return launch_policy_step(e, 1, (u32)seats, seats_per_game, TK_WEIGHTS(w1, b1, w2, b2, w3, b3), PolicyWeights{}, obs, action_out, logp_out,
                              value_out, feature_words_out, reward_out, done_out, trick_out, obs_out, flags, stream);
}

int tarok_policy_step_versus(tarok_env *e, int seats, const uint8_t *seats_per_game, const void *w1, const float *b1, const void *w2,
                             const float *b2, const void *w3, const float *b3, const void *v1, const float *c1, const void *v2,
                             const float *c2, const void *v3, const float *c3, const uint64_t *obs, uint8_t *action_out,
                             float *logp_out, float *value_out, uint64_t *feature_words_out, int16_t *reward_out, uint8_t *done_out,
                             uint16_t *trick_out, uint64_t *obs_out, int flags, void *stream) {
    if (!e || seats < 0 || seats > 15) return TAROK_EINVAL;       // (before the env is looked at, before any HIP call)
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !v1 || !c1 || !v2 || !c2 || !v3 || !c3) return TAROK_EINVAL;
    if (!obs || !action_out || !obs_out || obs == obs_out) return TAROK_EINVAL;
    return launch_policy_step(e, 2, (u32)seats, seats_per_game, TK_WEIGHTS(w1, b1, w2, b2, w3, b3), TK_WEIGHTS(v1, c1, v2, c2, v3, c3), obs,
                              action_out, logp_out, value_out, feature_words_out, reward_out, done_out, trick_out, obs_out, flags, stream);
}

int tarok_policy_step_pool(tarok_env *e, int seats, const uint8_t *seats_per_game, const void *w1, const float *b1, const void *w2,
                           const float *b2, const void *w3, const float *b3, int pool_size, const void *p1, const float *q1,
                           const void *p2, const float *q2, const void *p3, const float *q3, const uint8_t *group_net,
                           const uint64_t *obs, uint8_t *action_out, float *logp_out, float *value_out, uint64_t *feature_words_out,
                           int16_t *reward_out, uint8_t *done_out, uint16_t *trick_out, uint64_t *obs_out, int flags, void *stream) {
    if (!e || seats < 0 || seats > 15 || pool_size < 1 || pool_size > TAROK_POOL_MAX) return TAROK_EINVAL;   // (before any HIP call)
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !p1 || !q1 || !p2 || !q2 || !p3 || !q3) return TAROK_EINVAL;
    if (!obs || !action_out || !obs_out || obs == obs_out) return TAROK_EINVAL;
    return launch_policy_step(e, 3, (u32)seats, seats_per_game, TK_WEIGHTS(w1, b1, w2, b2, w3, b3), TK_WEIGHTS(p1, q1, p2, q2, p3, q3), obs,
                              action_out, logp_out, value_out, feature_words_out, reward_out, done_out, trick_out, obs_out, flags, stream,
                              (u32)pool_size, group_net);
}
#undef TK_WEIGHTS

int tarok_expand_features(tarok_env *e, int64_t n_samples, const uint64_t *feature_words, const int64_t *index,
                          void *features_out, void *stream) {
    if (!e || n_samples <= 0 || !feature_words || !features_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_expand_features, grid_for(n_samples * 32), dim3(TK_BLOCK), 0, (hipStream_t)stream, n_samples,
                       (const u64 *)feature_words, index, (uint4 *)features_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_ppo_loss(tarok_env *e, int64_t n_samples, const void *out_bf16, const uint64_t *obs, const int64_t *action,
                   const float *logp_old, const float *advantage, const float *ret, const float *weight, float clip,
                   float vf_coef, float ent_coef, const float *inv_weight_sum, void *dout_bf16, float *partial_out, void *stream) {
    if (!e || n_samples <= 0 || !out_bf16 || !obs || !action || !logp_old || !advantage || !ret || !weight || !dout_bf16 ||
        !partial_out || !inv_weight_sum)
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_ppo_loss, grid_for(n_samples), dim3(TK_BLOCK), 0, (hipStream_t)stream, n_samples,
                       (const uint4 *)out_bf16, (const u64 *)obs, action, logp_old, advantage, ret, weight, clip, vf_coef,
                       ent_coef, inv_weight_sum, (uint4 *)dout_bf16, (float4 *)partial_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_targets_ref(tarok_env *e, int T, const uint64_t *obs_before, const uint8_t *action, const uint16_t *trick,
                      const uint8_t *done, const int16_t *reward, const float *next_q, float final_reward_factor, float *dy_out,
                      uint8_t *meta_out, void *stream) {
    if (!e || T < 4 || (T & 3) || !obs_before || !action || !trick || !done || !reward || !dy_out || !meta_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    dim3 grid((unsigned)((e->n + TG_SLOTS - 1) / TG_SLOTS), (unsigned)(T / 4));
    hipLaunchKernelGGL(k_targets_ref, grid, dim3(256), 0, (hipStream_t)stream, e->n, T, (const u64 *)obs_before, action, trick, done,
                       reward, next_q, final_reward_factor, (float4 *)dy_out, meta_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// The one launch of the returns front end: a returns kernel (Monte-Carlo or GAE, seat-masked or not) and k_adv_stats on
// its block sums.  The masked kernel only where a mask can show: with the set 15 and no per-game sets it writes the
// bytes of the unmasked one.
static int launch_returns(tarok_env *e, int T, const uint8_t *done, const int16_t *reward, const uint64_t *obs, const float *logp,
                          const float *value, const uint8_t *action, float scale, int gae, float gamma, float lambda, int seats,
                          const uint8_t *seat_sets, float *rec, float *stats, float *scratch, void *stream) {
    if (!e || T < 1 || !done || !reward || !obs || !logp || !value || !action || !rec || !stats || !scratch) return TAROK_EINVAL;
    if (seats < 0 || seats > 15 || (gae != 0 && gae != 1)) return TAROK_EINVAL;
    if (gae && (!(gamma >= 0.f && gamma <= 1.f) || !(lambda >= 0.f && lambda <= 1.f))) return TAROK_EINVAL;      // (NaN fails both)
    HIPCHK(hipSetDevice(e->device));
    const dim3 grid = grid_for(e->n), block(TK_BLOCK);
    const hipStream_t st = (hipStream_t)stream;
    const u64 *w = (const u64 *)obs;
    float4 *r = (float4 *)rec, *part = (float4 *)scratch;
    const bool mask = seat_sets || seats != 15;
    if (gae && mask)
        hipLaunchKernelGGL(k_returns_gae_seats, grid, block, 0, st, e->n, T, done, reward, w, logp, value, action, scale, gamma,
                           gamma * lambda, (u32)seats, seat_sets, r, part);
    else if (gae)
        hipLaunchKernelGGL(k_returns_gae, grid, block, 0, st, e->n, T, done, reward, w, logp, value, action, scale, gamma, gamma * lambda, r, part);
    else if (mask)
        hipLaunchKernelGGL(k_returns_seats, grid, block, 0, st, e->n, T, done, reward, w, logp, value, action, scale, (u32)seats, seat_sets, r, part);
    else
        hipLaunchKernelGGL(k_returns, grid, block, 0, st, e->n, T, done, reward, w, logp, value, action, scale, r, part);
    hipLaunchKernelGGL(k_adv_stats, dim3(1), block, 0, st, (int)grid.x, (int64_t)T * e->n, (const float4 *)part, (float4 *)stats);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_learn_returns(tarok_env *e, int T, const uint8_t *done, const int16_t *reward, const uint64_t *obs, const float *logp,
                        const float *value, const uint8_t *action, float reward_scale, float *rec_out, float *stats_out,
                        float *scratch, void *stream) {
    return launch_returns(e, T, done, reward, obs, logp, value, action, reward_scale, 0, 1.f, 1.f, 15, nullptr, rec_out, stats_out, scratch, stream);
}

int tarok_learn_returns_gae(tarok_env *e, int T, const uint8_t *done, const int16_t *reward, const uint64_t *obs, const float *logp,
                            const float *value, const uint8_t *action, float reward_scale, float gamma, float lambda, float *rec_out,
                            float *stats_out, float *scratch, void *stream) {
    return launch_returns(e, T, done, reward, obs, logp, value, action, reward_scale, 1, gamma, lambda, 15, nullptr, rec_out, stats_out, scratch, stream);
}

int tarok_learn_returns_seats(tarok_env *e, int T, const uint8_t *done, const int16_t *reward, const uint64_t *obs, const float *logp,
                              const float *value, const uint8_t *action, float reward_scale, int gae, float gamma, float lambda,
                              int seats, const uint8_t *seats_per_game, float *rec_out, float *stats_out, float *scratch, void *stream) {
    return launch_returns(e, T, done, reward, obs, logp, value, action, reward_scale, gae, gamma, lambda, seats, seats_per_game, rec_out,
                          stats_out, scratch, stream);
}

// scratch of tarok_learn_select: tile_off [tiles] i64, then tile_cnt [tiles] u32 (rounded up to 16 bytes)
static inline int64_t select_tiles(int64_t M) { return (M + TAROK_LEARN_SELECT_TILE - 1) / TAROK_LEARN_SELECT_TILE; }
int64_t tarok_learn_select_scratch_bytes(int64_t M) {
    if (M < 1) return 0;
    return (select_tiles(M) * 12 + 15) / 16 * 16;
}

int tarok_learn_select(tarok_env *e, int64_t M, const float *rec, int64_t *index_out, int64_t *count_out, void *scratch, void *stream) {
    if (!e || M < 1 || !rec || !index_out || !count_out || !scratch) return TAROK_EINVAL;
    const int64_t tiles = select_tiles(M);
    if (tiles > 0x7FFFFFFF) return TAROK_EINVAL;              // (one workgroup per tile: the grid's first dimension)
    HIPCHK(hipSetDevice(e->device));
    int64_t *tile_off = (int64_t *)scratch;
    u32 *tile_cnt = (u32 *)(tile_off + tiles);
    hipLaunchKernelGGL(k_select_count, dim3((unsigned)tiles), dim3(TK_BLOCK), 0, (hipStream_t)stream, M, (const float4 *)rec, tile_cnt);
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(TK_BLOCK), 0, (hipStream_t)stream, tiles, (const u32 *)tile_cnt, tile_off, count_out);
    hipLaunchKernelGGL(k_select_scatter, dim3((unsigned)tiles), dim3(TK_BLOCK), 0, (hipStream_t)stream, M, (const float4 *)rec,
                       (const int64_t *)tile_off, index_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

// tarok_learn_chain and tarok_learn_chain_distill: one launcher, the kernel's instantiation chosen by DISTILL
extern "C++" {
template <bool DISTILL>
static int launch_learn_chain(tarok_env *e, int64_t B, const uint64_t *feature_words, const int64_t *index, const float *rec,
                              const float *stats, float clip, float vf_coef, float ent_coef, const void *w1, const float *b1,
                              const void *w2, const float *b2, const void *w3, const float *b3, const void *w3t, const void *w2t,
                              uint64_t *Xw, void *H1, void *H2, void *dOut, void *dH2, void *dH1, float *scratch, float *terms_out,
                              float *running, const void *target, float distill_coef, float *distill_scratch, float *distill_out,
                              float *distill_running, void *stream) {
    if (!e || B < 1 || !feature_words || !rec || !stats || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w3t || !w2t || !Xw || !H1 || !H2 ||
        !dOut || !dH2 || !dH1 || !scratch || !terms_out)
        return TAROK_EINVAL;
    if (DISTILL && (!target || !distill_scratch || !distill_out || !(distill_coef == distill_coef) || distill_coef > 3.0e38f || distill_coef < -3.0e38f))
        return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    std::conditional_t<DISTILL, LearnArgsDistill, LearnArgs> a;
    a.B = B; a.words = (const u64 *)feature_words; a.index = index; a.rec = (const float4 *)rec; a.stats = (const float4 *)stats;
    a.clip = clip; a.vf_coef = vf_coef; a.ent_coef = ent_coef;
    a.w1 = (const __bf16 *)w1; a.w2 = (const __bf16 *)w2; a.w3 = (const __bf16 *)w3; a.w3t = (const __bf16 *)w3t; a.w2t = (const __bf16 *)w2t;
    a.b1 = b1; a.b2 = b2; a.b3 = b3;
    a.Xw = (ulonglong2 *)Xw;
    a.H1 = (uint4 *)H1; a.H2 = (uint4 *)H2; a.dH2 = (uint4 *)dH2; a.dH1 = (uint4 *)dH1; a.dOut = (uint2 *)dOut;
    a.part = (float4 *)scratch;
    unsigned blocks = (unsigned)((B + LN_M - 1) / LN_M);
    a.stamps = stamps_for(e, 8 * (size_t)blocks);       // (eight stamps per workgroup: a buffer sized for the step kernels gets none)
    if constexpr (DISTILL) { a.target = (const uint2 *)target; a.distill_coef = distill_coef; a.dpart = (float2 *)distill_scratch; }
    hipLaunchKernelGGL(k_learn_chain<DISTILL>, dim3(blocks), dim3(LN_CHAIN_THREADS), 0, (hipStream_t)stream, a);
    if constexpr (DISTILL)
        hipLaunchKernelGGL(k_learn_terms_distill, dim3(1), dim3(TK_BLOCK), 0, (hipStream_t)stream, (int)blocks, (const float4 *)scratch,
                           (const float2 *)distill_scratch, (float4 *)terms_out, (float4 *)running, (float2 *)distill_out,
                           (float2 *)distill_running);
    else
        hipLaunchKernelGGL(k_learn_terms, dim3(1), dim3(TK_BLOCK), 0, (hipStream_t)stream, (int)blocks, (const float4 *)scratch,
                           (float4 *)terms_out, (float4 *)running);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}
}  // extern "C++"

int tarok_learn_chain(tarok_env *e, int64_t B, const uint64_t *feature_words, const int64_t *index, const float *rec,
                      const float *stats, float clip, float vf_coef, float ent_coef, const void *w1, const float *b1,
                      const void *w2, const float *b2, const void *w3, const float *b3, const void *w3t, const void *w2t,
                      uint64_t *Xw, void *H1, void *H2, void *dOut, void *dH2, void *dH1, float *scratch, float *terms_out,
                      float *running, void *stream) {
    return launch_learn_chain<false>(e, B, feature_words, index, rec, stats, clip, vf_coef, ent_coef, w1, b1, w2, b2, w3, b3, w3t, w2t, Xw,
                                     H1, H2, dOut, dH2, dH1, scratch, terms_out, running, nullptr, 0.f, nullptr, nullptr, nullptr, stream);
}

int tarok_learn_chain_distill(tarok_env *e, int64_t B, const uint64_t *feature_words, const int64_t *index, const float *rec,
                              const float *stats, float clip, float vf_coef, float ent_coef, const void *w1, const float *b1,
                              const void *w2, const float *b2, const void *w3, const float *b3, const void *w3t, const void *w2t,
                              uint64_t *Xw, void *H1, void *H2, void *dOut, void *dH2, void *dH1, float *scratch, float *terms_out,
                              float *running, const void *target, float distill_coef, float *distill_scratch, float *distill_out,
                              float *distill_running, void *stream) {
    return launch_learn_chain<true>(e, B, feature_words, index, rec, stats, clip, vf_coef, ent_coef, w1, b1, w2, b2, w3, b3, w3t, w2t, Xw,
                                    H1, H2, dOut, dH2, dH1, scratch, terms_out, running, target, distill_coef, distill_scratch, distill_out,
                                    distill_running, stream);
}

// chunks per layer of k_learn_dw: one workgroup per CU in all.  A tile costs a workgroup about the same in every
// layer (per-tile overheads, not bytes or MFMAs, set its time at this size), a little more where both operands are
// 256 wide (layer 2) or the input is expanded from feature words (layer 1), less where the gradient is 64 wide
// (layer 3): shares 96 : 108 : 52 (same-box A/B of six settings: profiles/r03_learner_steps.txt).
static inline void learn_chunks(tarok_env *e, u32 &c2, u32 &c1, u32 &c3) {
    if (!e->n_cus) {
        hipDeviceProp_t pr;
        e->n_cus = hipGetDeviceProperties(&pr, e->device) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
    }
    u32 total = (u32)e->n_cus < 8 ? 8 : (u32)e->n_cus;
    c2 = total * 96 / 256; c1 = total * 108 / 256; c3 = total - c2 - c1;
}

int64_t tarok_learn_workspace_bytes(tarok_env *e) {
    if (!e) return 0;
    u32 c2, c1, c3;
    learn_chunks(e, c2, c1, c3);
    return (int64_t)sizeof(float) * ((int64_t)(c2 + c1) * 65792 + (int64_t)c3 * 16448);
}

int tarok_learn_dw(tarok_env *e, int64_t B, const uint64_t *Xw, const void *H1, const void *H2,
                   const void *dOut, const void *dH2, const void *dH1, const float *terms, void *workspace, float *grad_out,
                   void *stream) {
    if (!e || B < 1 || !Xw || !H1 || !H2 || !dOut || !dH2 || !dH1 || !terms || !workspace || !grad_out) return TAROK_EINVAL;
    if (B > TAROK_LEARN_MAX_BATCH) return TAROK_EINVAL;       // (k_learn_dw addresses its arrays through 32-bit buffer offsets: 512 B rows)
    HIPCHK(hipSetDevice(e->device));
    u32 c2, c1, c3;
    learn_chunks(e, c2, c1, c3);
    hipLaunchKernelGGL(k_learn_dw, dim3(c2 + c1 + c3), dim3(TK_BLOCK), 0, (hipStream_t)stream, B, c2, c1, c3, (const u64 *)Xw,
                       (const uint4 *)H1, (const uint4 *)H2, (const uint4 *)dOut, (const uint4 *)dH2, (const uint4 *)dH1,
                       (float *)workspace);
    hipLaunchKernelGGL(k_learn_reduce, dim3((LN_P + TK_BLOCK - 1) / TK_BLOCK), dim3(TK_BLOCK), 0, (hipStream_t)stream, c2, c1, c3,
                       (const float *)workspace, (const float4 *)terms, grad_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_learn_adam(tarok_env *e, float *param, const float *grad, float *m, float *v, int32_t *step, float lr, float beta1,
                     float beta2, float eps, float max_norm, void *w1, void *w2, void *w3, void *w3t, void *w2t, float *gnorm_out,
                     int apply, void *stream) {
    if (!e || !param || (apply && (!grad || !m || !v || !step))) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    AdamArgs a;
    a.param = param; a.grad = const_cast<float *>(grad); a.m = m; a.v = v; a.step = step;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.max_norm = max_norm;
    a.w1 = (__bf16 *)w1; a.w2 = (__bf16 *)w2; a.w3 = (__bf16 *)w3; a.w3t = (__bf16 *)w3t; a.w2t = (__bf16 *)w2t;
    a.gnorm = gnorm_out; a.apply = apply;
    a.sumsq = e->adam_sumsq;
    if (apply) hipLaunchKernelGGL(k_learn_gnorm, dim3(LN_ADAM_BLOCKS), dim3(LN_ADAM_BLOCK), 0, (hipStream_t)stream, grad, e->adam_sumsq, step);
    hipLaunchKernelGGL(k_learn_adam, dim3(LN_ADAM_BLOCKS), dim3(LN_ADAM_BLOCK), 0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_get_state(tarok_env *e, uint64_t *lanes_out, void *stream) {
    if (!e || !lanes_out) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_get_state, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->s01, e->s23,
                       (u64 *)lanes_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_set_state(tarok_env *e, const uint64_t *lanes_in, void *stream) {
    if (!e || !lanes_in) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_set_state, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, (const u64 *)lanes_in,
                       e->s01, e->s23, e->cnt);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

int tarok_get_counters(tarok_env *e, uint32_t *episode_out, int32_t *score_sum_out, void *stream) {
    if (!e) return TAROK_EINVAL;
    HIPCHK(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_counters, grid_for(e->n), dim3(TK_BLOCK), 0, (hipStream_t)stream, e->n, e->cnt, episode_out,
                       (int4 *)score_sum_out);
    HIPCHK(hipGetLastError());
    return TAROK_OK;
}

}  // extern "C"
