// Learner side of the self-play loop (SURVEY 8f row 4; BASELINE config 4): the policy-gradient update of the
// 256-256-256-64 MLP policy as five kernels per minibatch instead of ~60 framework launches.  Included by
// tarok_env.hip (one translation unit: the forward layers share the policy kernels' fragment layout).
// Build-owned: the reference trains a double-Q LSTM agent with pytorch-lightning (Igralec.py:545-714; network
// shapes train.py:4-27) and has no PPO, so nothing here is pinned to it; the tests compare every stage with
// float32 torch autograd on the same bf16 weights.
//
//   k_returns      per slot, backwards over the rollout: every card is credited with its seat's final score of
//                  its game; packs the per-sample record the update gathers; sums for the advantage statistics
//   k_returns_gae  the same walk with per-seat GAE(gamma, lambda) returns bootstrapped from the seat's next decision
//   k_returns_seats, k_returns_gae_seats   the two walks with `known` masked by the learner's seats of the slot (training
//                  against a frozen opponent: the other seats' samples are somebody else's cards)
//   k_select_*     stable compaction of the known samples into an index list (count per tile, scan, scatter): the
//                  minibatches of k_learn_chain then hold the learner's samples only
//   k_learn_chain  one 128-sample tile per workgroup, activations in LDS: feature gather + expansion ->
//                  layer 1, 2, 3 (bf16 MFMA, f32 accumulate) -> clipped-surrogate / value / entropy loss and its
//                  gradient in the layer-3 accumulators -> dH2 = (dOut W3) . relu' -> dH1 = (dH2 W2) . relu'.
//                  Writes H1, H2, dOut, dH2, dH1 (bf16, row major) and the gathered feature words (minibatch order)
//                  for the weight gradients.
//   k_learn_dw     the three weight gradients dW = dH^T . H as ONE launch: every workgroup owns a whole
//                  256 x 256 (64 x 256) partial product over its chunk of the samples, operands staged row major
//                  in LDS and read TRANSPOSED (ds_read_b64_tr_b16: the contraction runs over the samples);
//                  bias gradients as column sums of the staged dH tile.
//   k_learn_reduce partial products -> one flat f32 gradient vector (scaled by 1 / sum of the sample weights)
//   k_learn_adam   gradient-norm clip + Adam on flat parameter / state vectors, and the bf16 fragment-order
//                  copies of the weights (and of their transposes, for the backward chain) that the next
//                  minibatch's kernels and the rollout read.  One workgroup.
#define LN_M 96                    // samples per tile of k_learn_chain: three 32-sample MFMA tiles — 75 KB of LDS, so that TWO
                                   // workgroups share a CU and one's epilogues, loss and gather run under the other's MFMAs
                                   // (128 samples: 100 KB, one workgroup per CU, 17 % of the MFMA rate)
#define LN_GT (LN_M / 32)
#define LN_LDD 72                  // dOut row stride in LDS (bf16 elements): 144 B
#define LN_P_W1 0
#define LN_P_B1 65536
#define LN_P_W2 65792
#define LN_P_B2 131328
#define LN_P_W3 131584
#define LN_P_B3 147968
#define LN_P 148032                // parameters of the 256-256-256-64 MLP, flat: W1 b1 W2 b2 W3 b3 (torch Linear layouts)
static_assert(LN_P == TAROK_MLP_PARAMS, "flat parameter vector");

// ---------------------------------------------------------------------------------------------------------------
// Returns.  done [T,N] u8, reward [T,N,4] i16 (valid where done), words [T,N] observation words (seat to move),
// logp / val [T,N] f32 from the rollout, act [T,N] u8.  rec [T,N] float4 = {logp_old, ret * scale, val, bits:
// card | known << 8} where known = the game the card belongs to ended inside the rollout.  part [blocks][4] =
// {sum known, sum adv, sum adv^2, 0} with adv = ret - val (f32, fixed order inside a block).
// MASK (k_returns_seats): known = that AND the seat to move is one of the learner's seats of the slot (`seat_sets[i]`, or
// `seats` for every slot: 4-bit sets as in tarok_policy_step_versus, bits 4..7 ignored).  The set is read once per slot
// and tested by a 32-bit shift; everything else of the record is written as without the mask.
#define TK_RETURNS_ARGS int64_t n, int T, const uint8_t *__restrict__ done, const int16_t *__restrict__ reward,                  \
                        const u64 *__restrict__ words, const float *__restrict__ logp, const float *__restrict__ val,        \
                        const uint8_t *__restrict__ act, float scale
#define TK_RETURNS_NAMES n, T, done, reward, words, logp, val, act, scale
template <bool MASK>
__device__ __forceinline__ void returns_walk(TK_RETURNS_ARGS, u32 seats, const uint8_t *__restrict__ seat_sets,
                                             float4 *__restrict__ rec, float4 *__restrict__ part) {
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    float s_n = 0.f, s_a = 0.f, s_q = 0.f;
    if (i < n) {
        u64 cur = 0;
        bool have = false;
        const u32 set = MASK ? (seat_sets ? (u32)seat_sets[i] : seats) : 15u;
#pragma unroll 4                                             // (four lock-steps' loads in flight: the walk is latency bound)
        for (int t = T - 1; t >= 0; t--) {
            int64_t j = (int64_t)t * n + i;
            if (done[j]) { cur = reinterpret_cast<const u64 *>(reward)[j]; have = true; }
            u32 seat = (u32)(words[j] >> TAROK_OBS_SEAT_SHIFT) & 3u;
            float r = (float)(int16_t)((cur >> (16 * seat)) & 0xFFFF) * scale;
            float v = val[j];
            const bool known = MASK ? have && ((set >> seat) & 1u) : have;
            rec[j] = make_float4(logp[j], r, v, __uint_as_float((u32)act[j] | (known ? 256u : 0u)));
            if (known) { float a = r - v; s_n += 1.f; s_a += a; s_q += a * a; }
        }
    }
    block_sum3(s_n, s_a, s_q, part);
}
TK_KERNEL(TK_BLOCK, 64) void k_returns(TK_RETURNS_ARGS, float4 *__restrict__ rec, float4 *__restrict__ part) {
    TK_VGPR_TOP(64, 63);
    returns_walk<false>(TK_RETURNS_NAMES, 15u, nullptr, rec, part);
}
TK_KERNEL(TK_BLOCK, 64) void k_returns_seats(TK_RETURNS_ARGS, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                           float4 *__restrict__ rec, float4 *__restrict__ part) {
    TK_VGPR_TOP(64, 63);
    returns_walk<true>(TK_RETURNS_NAMES, seats, seat_sets, rec, part);
}

// Returns by GAE(gamma, lambda), per seat.  Arrays and rec / part as k_returns; the walk keeps, for each of the four seats,
// what the seat's NEXT decision inside the rollout left behind: have (there is one, or the game ended), next_v (its
// value), next_adv (its advantage) and pend_r (the seat's scaled final score if its game ended in between, else 0).
// At lock-step t, seat s to move, v = val[t]:
//     done[t]:   for every seat pend_r = reward[t][seat] * scale, next_v = next_adv = 0, have = true
//                (the steps after t belong to the slot's next game and are behind us)
//     have[s]:   delta = pend_r[s] + gamma * next_v[s] - v,  A = delta + gamma * lambda * next_adv[s],  known
//     else:      A = 0, not known: the seat's last decision of a game that is unfinished when the rollout ends
//     rec[t].y = A + v;  then next_v[s] = v, next_adv[s] = A, pend_r[s] = 0, have[s] = true (an unknown tail sample is
//                still the bootstrap of the seat's earlier decisions)
// gamma discounts per DECISION OF THE SEAT (its next card is one step away, four lock-steps later), not per lock-step.
// At most one sample per seat and slot stays unknown: stats[2] >= 1 - 4 / T.  gl = gamma * lambda (f32 product).
// The seat's state is picked by compare / select over four named registers (a runtime-indexed array would live in
// scratch memory), and the scores are loaded as four shorts: no 64-bit shift by a variable amount (DESIGN.md section 3).
// MASK (k_returns_gae_seats): the record's known bit and the sums are ANDed with the learner's seat set of the slot as in
// returns_walk; the walk's own state (A, have, next_v, next_adv, pend_r of every seat) is kept as without the mask — a
// seat's chain reads that seat's values only, so a learner seat's returns are the unmasked ones.
template <bool MASK>
__device__ __forceinline__ void returns_gae_walk(TK_RETURNS_ARGS, float gamma, float gl, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                 float4 *__restrict__ rec, float4 *__restrict__ part) {
    int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    float s_n = 0.f, s_a = 0.f, s_q = 0.f;
    if (i < n) {
        const u32 set = MASK ? (seat_sets ? (u32)seat_sets[i] : seats) : 15u;
        float nv[4] = {0.f, 0.f, 0.f, 0.f}, na[4] = {0.f, 0.f, 0.f, 0.f}, pr[4] = {0.f, 0.f, 0.f, 0.f};   // (constant indices only)
        u32 have = 0;                                        // bit s: seat s
#pragma unroll 4                                             // (four lock-steps' loads in flight: the walk is latency bound)
        for (int t = T - 1; t >= 0; t--) {
            int64_t j = (int64_t)t * n + i;
            if (done[j]) {
                short4 rw = reinterpret_cast<const short4 *>(reward)[j];
                pr[0] = (float)rw.x * scale; pr[1] = (float)rw.y * scale; pr[2] = (float)rw.z * scale; pr[3] = (float)rw.w * scale;
#pragma unroll
                for (int k = 0; k < 4; k++) { nv[k] = 0.f; na[k] = 0.f; }
                have = 15u;
            }
            u32 seat = (u32)(words[j] >> TAROK_OBS_SEAT_SHIFT) & 3u;
            float v = val[j];
            float p = pr[3], nvs = nv[3], nas = na[3];
#pragma unroll
            for (int k = 0; k < 3; k++) { bool m = seat == (u32)k; p = m ? pr[k] : p; nvs = m ? nv[k] : nvs; nas = m ? na[k] : nas; }
            bool known = (have >> seat) & 1u;
            float a = known ? (p + gamma * nvs - v) + gl * nas : 0.f;
            const bool mine = MASK ? known && ((set >> seat) & 1u) : known;
            rec[j] = make_float4(logp[j], a + v, v, __uint_as_float((u32)act[j] | (mine ? 256u : 0u)));
#pragma unroll
            for (int k = 0; k < 4; k++) { bool m = seat == (u32)k; pr[k] = m ? 0.f : pr[k]; nv[k] = m ? v : nv[k]; na[k] = m ? a : na[k]; }
            have |= 1u << seat;
            if (mine) { s_n += 1.f; s_a += a; s_q += a * a; }
        }
    }
    block_sum3(s_n, s_a, s_q, part);
}
TK_KERNEL(TK_BLOCK, 64) void k_returns_gae(TK_RETURNS_ARGS, float gamma, float gl, float4 *__restrict__ rec, float4 *__restrict__ part) {
    TK_VGPR_TOP(64, 63);
    returns_gae_walk<false>(TK_RETURNS_NAMES, gamma, gl, 15u, nullptr, rec, part);
}
TK_KERNEL(TK_BLOCK, 64) void k_returns_gae_seats(TK_RETURNS_ARGS, float gamma, float gl, u32 seats, const uint8_t *__restrict__ seat_sets,
                                                               float4 *__restrict__ rec, float4 *__restrict__ part) {
    TK_VGPR_TOP(64, 63);
    returns_gae_walk<true>(TK_RETURNS_NAMES, gamma, gl, seats, seat_sets, rec, part);
}

// Column sums of `blocks` float4 partials by one workgroup, in double and in a fixed order (strided accumulate per thread,
// LDS tree): afterwards red[c][0] = the sum of column c, for thread 0.
// (E = 2: two more columns, C and C + 1, from a second array of float2 partials: the distillation term's)
template <int C, int E = 0>
__device__ __forceinline__ void part_column_sums(int blocks, const float4 *__restrict__ part, double (&red)[C + E][TK_BLOCK],
                                                 const float2 *__restrict__ extra = nullptr) {
    static_assert(E == 0 || E == 2, "no extra columns, or one float2 per block");
    double a[C + E] = {};
    for (int k = threadIdx.x; k < blocks; k += TK_BLOCK) {
        float4 p = part[k];
        const float col[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int c = 0; c < C; c++) a[c] += col[c];
        if constexpr (E == 2) { float2 x = extra[k]; a[C] += x.x; a[C + 1] += x.y; }
    }
#pragma unroll
    for (int c = 0; c < C + E; c++) red[c][threadIdx.x] = a[c];
    __syncthreads();
    for (int s = TK_BLOCK / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int c = 0; c < C + E; c++) red[c][threadIdx.x] += red[c][threadIdx.x + s];
        }
        __syncthreads();
    }
}

// stats = {mean, 1 / std, known fraction, 0} of the advantages from the returns kernels' block sums (one workgroup)
TK_KERNEL(TK_BLOCK, 64) void k_adv_stats(int blocks, int64_t total, const float4 *__restrict__ part, float4 *__restrict__ stats) {
    TK_VGPR_TOP(64, 63);
    __shared__ double red[3][TK_BLOCK];
    part_column_sums<3>(blocks, part, red);
    if (threadIdx.x == 0) {
        double cnt = red[0][0] < 1.0 ? 1.0 : red[0][0];
        double mean = red[1][0] / cnt;
        double var = red[2][0] / cnt - mean * mean;
        double sd = sqrt(var > 0 ? var : 0);
        if (sd < 1e-6) sd = 1e-6;
        stats[0] = make_float4((float)mean, (float)(1.0 / sd), (float)(red[0][0] / (double)(total < 1 ? 1 : total)), 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Compaction of the known samples (tarok_learn_select): index_out[0 .. count) = the sample numbers j whose record has the
// known bit (bit 8 of rec[j].w), ascending.  Three stream-ordered launches and no workgroup that waits for another:
//   k_select_count    one workgroup per tile of TAROK_LEARN_SELECT_TILE samples: how many of them are known
//   k_select_scan     ONE workgroup: exclusive prefix sums of the tile counts (64 bit) and the total
//   k_select_scatter  one workgroup per tile: the known samples' numbers to index_out from the tile's prefix on
// A tile is SEL_ROUNDS rounds of 64 consecutive samples for each of the workgroup's four waves (wave w: samples
// [SEL_WAVE w, SEL_WAVE (w + 1)) of the tile), lane l of a round its l-th sample: the rank of a known sample inside its
// round is the number of known lanes below it (ballot + mbcnt), in front of it the wave's earlier rounds (popcounts of
// their ballots, the same in every lane), the tile's earlier waves (LDS) and the earlier tiles (the scan).  Both passes
// evaluate the same predicate on the same records, so every rank lies below the total.  Samples at or past M are not
// known.  Sample numbers and the byte offsets made of them are 64 bit throughout (rec of 2^28 samples is 4 GiB).
#define SEL_ROUNDS (TAROK_LEARN_SELECT_TILE / TK_BLOCK)
#define SEL_WAVE (64 * SEL_ROUNDS)
static_assert(TK_BLOCK == 256 && TAROK_LEARN_SELECT_TILE % TK_BLOCK == 0, "a tile is whole rounds of the four waves");
// the ballots of the wave's rounds (all loads in flight at once) and, bit r of `mine`, whether the lane's own sample of
// round r is known; returns how many of the wave's samples are known
__device__ __forceinline__ u32 select_ballots(int64_t M, const float4 *__restrict__ rec, int64_t wave0, u64 (&b)[SEL_ROUNDS], u32 &mine) {
    const u32 lane = threadIdx.x & 63;
    u32 w[SEL_ROUNDS];
#pragma unroll
    for (int r = 0; r < SEL_ROUNDS; r++) {
        int64_t j = wave0 + 64 * r + lane;
        w[r] = j < M ? reinterpret_cast<const u32 *>(rec + j)[3] : 0u;
    }
    u32 total = 0;
    mine = 0;
#pragma unroll
    for (int r = 0; r < SEL_ROUNDS; r++) {
        const u32 k = (w[r] >> 8) & 1u;
        mine |= k << r;
        b[r] = __ballot(k != 0u);
        total += (u32)__popcll(b[r]);
    }
    return total;
}
TK_KERNEL(TK_BLOCK, 64) void k_select_count(int64_t M, const float4 *__restrict__ rec, u32 *__restrict__ tile_cnt) {
    TK_VGPR_TOP(64, 63);
    __shared__ u32 wtot[TK_BLOCK / 64];
    const u32 wave = threadIdx.x >> 6;
    u64 b[SEL_ROUNDS];
    u32 mine;
    u32 total = select_ballots(M, rec, (int64_t)blockIdx.x * TAROK_LEARN_SELECT_TILE + (int64_t)wave * SEL_WAVE, b, mine);
    if ((threadIdx.x & 63) == 0) wtot[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
}
// thread t owns tiles [per t, per (t + 1)): their sum, an exclusive scan of the 256 sums in LDS, then the prefixes
TK_KERNEL(TK_BLOCK, 64) void k_select_scan(int64_t tiles, const u32 *__restrict__ tile_cnt, int64_t *__restrict__ tile_off,
                                                         int64_t *__restrict__ count_out) {
    TK_VGPR_TOP(64, 63);
    __shared__ int64_t sums[TK_BLOCK];
    const int64_t per = (tiles + TK_BLOCK - 1) / TK_BLOCK;
    const int64_t k0 = per * threadIdx.x < tiles ? per * threadIdx.x : tiles, k1 = k0 + per < tiles ? k0 + per : tiles;
    int64_t s = 0;
    for (int64_t k = k0; k < k1; k++) s += tile_cnt[k];
    sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int k = 0; k < TK_BLOCK; k++) { int64_t c = sums[k]; sums[k] = run; run += c; }
        count_out[0] = run;
    }
    __syncthreads();
    int64_t run = sums[threadIdx.x];
    for (int64_t k = k0; k < k1; k++) { tile_off[k] = run; run += tile_cnt[k]; }
}
TK_KERNEL(TK_BLOCK, 64) void k_select_scatter(int64_t M, const float4 *__restrict__ rec, const int64_t *__restrict__ tile_off,
                                                            int64_t *__restrict__ index_out) {
    TK_VGPR_TOP(64, 63);
    __shared__ u32 wtot[TK_BLOCK / 64];
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * TAROK_LEARN_SELECT_TILE + (int64_t)wave * SEL_WAVE;
    u64 b[SEL_ROUNDS];
    u32 mine;
    u32 total = select_ballots(M, rec, wave0, b, mine);
    if (lane == 0) wtot[wave] = total;
    __syncthreads();
    int64_t at = tile_off[blockIdx.x];
#pragma unroll
    for (u32 k = 0; k < TK_BLOCK / 64 - 1; k++) at += k < wave ? wtot[k] : 0u;
#pragma unroll
    for (int r = 0; r < SEL_ROUNDS; r++) {
        const u32 below = __builtin_amdgcn_mbcnt_hi((u32)(b[r] >> 32), __builtin_amdgcn_mbcnt_lo((u32)b[r], 0u));
        if ((mine >> r) & 1u) index_out[at + below] = wave0 + 64 * r + lane;
        at += (u32)__popcll(b[r]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// One layer of the chain in the transposed form of mlp_hidden: D[feature][sample] = Wf[feature][k] * B^T[k][sample],
// KSTEPS k-steps of 16, for the wave's 64 features x LN_M samples.  Wf = fragment-order weights (tile-major:
// [feature / 32][k-step][lane][8]), Bsrc = LDS rows [sample][k] with row stride ldb.
// `tail()` runs in the k-step that has issued the layer's LAST weight loads: the place for the stores of the tile before (see
// k_learn_chain).
struct ChainNoTail { __device__ __forceinline__ void operator()() const {} };
template <int KSTEPS, class Tail = ChainNoTail>
__device__ __forceinline__ void chain_gemm(f32x16 (&acc)[2][LN_GT], const __bf16 *__restrict__ Bsrc, int ldb, const __bf16 *__restrict__ w, u32 wave,
                                           Tail tail = Tail()) {
    u32 lane = __lane_id(), r = lane & 31, h = lane >> 5;
    // the wave's 2 x KSTEPS weight fragments as a raw buffer: one resource, the lane's 16 bytes as the only vector offset,
    // the fragment's number in the scalar / immediate offset — no address arithmetic per load
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<__bf16 *>(w) + (size_t)__builtin_amdgcn_readfirstlane(wave) * (2 * KSTEPS * 64 * 8), 0, 2 * KSTEPS * 1024, 0x00020000);
    auto wfrag = [&](int f) __attribute__((always_inline)) {
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, (int)(lane * 16), f * 1024, 0));
    };
#pragma unroll
    for (int ft = 0; ft < 2; ft++)
#pragma unroll
        for (int gt = 0; gt < LN_GT; gt++)
#pragma unroll
            for (int j = 0; j < 16; j++) acc[ft][gt][j] = 0.f;
    constexpr int AHEAD = KSTEPS < 4 ? KSTEPS : 4;
    bf16x8 wq[AHEAD][2];
#pragma unroll
    for (int d = 0; d < AHEAD; d++)
#pragma unroll
        for (int ft = 0; ft < 2; ft++) wq[d][ft] = wfrag(ft * KSTEPS + d);
    bf16x8 xn[LN_GT];
#pragma unroll
    for (int gt = 0; gt < LN_GT; gt++) xn[gt] = *reinterpret_cast<const bf16x8 *>(Bsrc + (32 * gt + r) * ldb + 8 * h);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kk = 0; kk < KSTEPS; kk++) {
        bf16x8 x[LN_GT];
#pragma unroll
        for (int gt = 0; gt < LN_GT; gt++) x[gt] = xn[gt];
        bf16x8 wc[2] = {wq[kk % AHEAD][0], wq[kk % AHEAD][1]};
        if (kk + AHEAD < KSTEPS) {
#pragma unroll
            for (int ft = 0; ft < 2; ft++) wq[kk % AHEAD][ft] = wfrag(ft * KSTEPS + kk + AHEAD);
        }
        if (kk + 1 < KSTEPS) {
#pragma unroll
            for (int gt = 0; gt < LN_GT; gt++) xn[gt] = *reinterpret_cast<const bf16x8 *>(Bsrc + (32 * gt + r) * ldb + 16 * (kk + 1) + 8 * h);
        }
        if (kk == KSTEPS - AHEAD) tail();
#pragma unroll
        for (int ft = 0; ft < 2; ft++)
#pragma unroll
            for (int gt = 0; gt < LN_GT; gt++) acc[ft][gt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc[ft], x[gt], acc[ft][gt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);     // (keep this k-step's loads here: see mlp_hidden)
    }
}

// What the chain writes for k_learn_dw (0.85 GB per minibatch, read once by the next kernel, far more than the caches hold) leaves
// as NON-TEMPORAL stores and is read with non-temporal loads — as ordinary stores the tiles sat in the L2s as dirty lines whose
// write-back ran into k_learn_dw's reads: k_learn_dw 231 -> 174 us per minibatch (profiles/r04_learner_steps.txt (5)).
typedef __attribute__((ext_vector_type(4))) unsigned int ln_u32x4;
// Cache policy of the stores k_learn_chain leaves for k_learn_dw (buffer stores: the policy bits are an immediate of the
// builtin — 0 plain, 2 non-temporal, 16 `sc1` = write-through).  Same box, us per minibatch, k_learn_chain | k_learn_dw:
// non-temporal 276 | 182, plain 278 | 202, write-through 281 | 200 (profiles/r04_learner_steps.txt).
#define LN_STORE_AUX 2
// rows [row0, row0 + valid) x `row_bytes` of a row-major array as a raw buffer: a store past `valid` rows is dropped by the
// bounds check of the buffer instruction (no row test in the code)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t chain_rows(void *first_row, int64_t row0, int64_t nrows, u32 row_bytes) {
    const u32 valid = nrows - row0 < LN_M ? (u32)(nrows - row0) : (u32)LN_M;
    return __builtin_amdgcn_make_buffer_rsrc(first_row, 0, (int)(valid * row_bytes), 0x00020000);
}
__device__ __forceinline__ void chain_store16(__amdgpu_buffer_rsrc_t rs, u32 byte_offset, uint4 v) {
    ln_u32x4 t = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(t, rs, (int)byte_offset, 0, LN_STORE_AUX);
}
// the LN_M x 256 activation tile in LDS -> rows [row0, row0 + LN_M) of a row-major [.,256] bf16 array (full 512-byte rows)
__device__ __forceinline__ void chain_store_tile(const __bf16 *__restrict__ X, uint4 *__restrict__ out, int64_t row0, int64_t nrows, u32 tid) {
    __amdgpu_buffer_rsrc_t rs = chain_rows(out + row0 * 32, row0, nrows, 512);
#pragma unroll
    for (int it = 0; it < LN_M / 8; it++) {
        u32 s = it * 8 + (tid >> 5), chunk = tid & 31;
        chain_store16(rs, (s * 32 + chunk) * 16, *reinterpret_cast<const uint4 *>(X + s * PM_LD + 8 * chunk));
    }
}

// Packed epilogue arithmetic: the chain's vector pipe is busier than its matrix pipe (profiles/r04_learner_sq_counters.txt), and a
// third of its vector instructions are epilogues.  Two floats per instruction where the ISA has the form: bias add
// (v_pk_add_f32), conversion (v_cvt_pk_bf16_f32); ReLU AFTER the conversion as a signed 16-bit max per half (a negative bf16
// is a negative int16, -0.0 included), which gives the same bits as converting max(x, 0); "is it positive" = "is its bf16
// non-zero" (ln_nonzero_u16x2).
typedef float ln_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 ln_bf16x2 __attribute__((ext_vector_type(2)));
typedef short ln_s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32 ln_relu_bf16x2(float a0, float a1, float b0, float b1) {       // bf16 pair of relu(a + b)
    ln_f32x2 v = ln_f32x2{a0, a1} + ln_f32x2{b0, b1};
    ln_s16x2 p = __builtin_bit_cast(ln_s16x2, __builtin_convertvector(v, ln_bf16x2));
    return __builtin_bit_cast(u32, __builtin_elementwise_max(p, ln_s16x2{0, 0}));
}
__device__ __forceinline__ u32 ln_bf16x2_of(float a0, float a1) {
    return __builtin_bit_cast(u32, __builtin_convertvector(ln_f32x2{a0, a1}, ln_bf16x2));
}
// 1 in every half of a pair of NON-NEGATIVE bf16 (< 0x8000) that is not zero: bit 15 of (half + 0x7FFF), no carry between the
// halves.  (As min(u16, 1) the compiler turns it into a compare and a select per half.)
__device__ __forceinline__ u32 ln_nonzero_u16x2(u32 x) { return ((x + 0x7FFF7FFFu) >> 15) & 0x00010001u; }

// AND mask of a bf16 pair from two mask bits (bit 0 -> low half, bit 1 -> high half)
__device__ __forceinline__ u32 ln_pair_mask(u32 two_bits) {
    return __umul24((two_bits | (two_bits << 15)) & 0x00010001u, 0xFFFFu);
}

struct LearnArgs {
    int64_t B;                                   // samples of this minibatch
    const u64 *words; const int64_t *index;      // feature words [M][4] of the rollout; sample j = row index[j] (NULL: row j)
    const float4 *rec;                           // per-sample record [M] (k_returns)
    const float4 *stats;                         // {advantage mean, 1 / std, ., .}
    float clip, vf_coef, ent_coef;
    const __bf16 *w1, *w2, *w3, *w3t, *w2t;      // fragment order (k_learn_adam)
    const float *b1, *b2, *b3;
    ulonglong2 *Xw;                              // [B][4] u64: the samples' feature words in minibatch order (for k_learn_dw's layer 1)
    uint4 *H1, *H2, *dH2, *dH1;                  // [B][256] bf16
    uint2 *dOut;                                 // [B][64] bf16
    float4 *part;                                // [blocks] {sum w pi, sum w v, sum w H, sum w}
    u64 *stamps;                                 // diagnostics (tarok_debug_stamps): [blocks][8] shader-clock stamps of the phases, or NULL
};
// tarok_learn_chain_distill: the same and the playout teacher's target rows.  A struct of its own, so that the kernel
// arguments of the instantiation without the term are LearnArgs, byte for byte
struct LearnArgsDistill : LearnArgs {
    const uint2 *target;                         // [M][64] bf16 as 16 x 8 bytes per row; row = sample number, as for rec
    float distill_coef;
    float2 *dpart;                               // [blocks] {sum w ce, sum w S}
};

// Two workgroups share a CU (75 KB of LDS, 186 VGPRs: two waves per SIMD): one's gather, epilogues, loss and tile
// stores run under the other's MFMAs.  (A fifth, store-only wave per workgroup was tried — on gfx9 `vmcnt` counts loads
// and stores together, in order, so a wave that has just stored a tile waits for those stores at its next weight
// fragment — but five waves of 186 registers leave room for ONE workgroup per CU: 552 us against 499 us per
// minibatch, profiles/r03_learner_steps.txt.)
// DISTILL (tarok_learn_chain_distill): the cross-entropy of the policy against a target row q per sample, beside the other
// three terms: ce = -sum_c q_c log p_c over the LEGAL cards c (q of every other column is dropped by a select: a NaN there
// reaches nothing), S = sum_c q_c, d ce / d logit_c = S p_c - q_c.  The lane that holds outputs 32 ft + 8 q + 4 h .. + 3 of a
// sample loads exactly those eight 8-byte pieces of the sample's target row — the layout of its D store — in the gather
// phase: the row number comes from `index` by a load at the kernel's top, the eight loads leave behind the gather's own and
// in front of every tile store, and the first weight fragment of layer 1, which the wave waits for anyway, retires them
// (vmcnt counts in order): the loss phase, two layers later, never waits for them.  Sixteen registers held until then.
// Everything of the term sits under `if constexpr (DISTILL)`; tarok_learn_chain launches k_learn_chain<false>.  (That
// instantiation has the registers, LDS bytes and matrix / memory instructions of the kernel before the term existed, but not
// its exact instruction stream: figures and the timing that goes with them in DESIGN.md section 8.5.)
#define LN_CHAIN_THREADS TK_BLOCK
template <bool DISTILL>
TK_KERNEL(LN_CHAIN_THREADS, 256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_learn_chain(std::conditional_t<DISTILL, LearnArgsDistill, LearnArgs> a) {
    TK_VGPR_TOP(256, 255);
    __shared__ __attribute__((aligned(16))) __bf16 X[LN_M * PM_LD];
    __shared__ __attribute__((aligned(16))) __bf16 D[LN_M * LN_LDD];
    __shared__ __attribute__((aligned(16))) u64 ext[LN_M][4];
    __shared__ float4 recs[LN_M];
    // layer-1 ReLU mask: one nibble (4 consecutive features) per byte, [feature quad][sample]: the 32 lanes of a half
    // wave hold 32 consecutive samples of one feature quad, so they write 32 consecutive bytes (round 3's [sample][quad]
    // put them 64 bytes apart — an eight-way bank conflict on every one of the 24 byte stores of a lane: k_learn_chain
    // 320 -> 302 us per minibatch, profiles/r04_learner_steps.txt)
    __shared__ uint8_t mask1[64][LN_M];
    __shared__ float red[DISTILL ? 6 : 4][TK_BLOCK / 64];
    __shared__ __attribute__((aligned(16))) float bias_s[580];        // b1 | b2 | b3 | stats: read from LDS, so that no epilogue waits for a
                                                                       // vector-memory load (behind the tile stores in flight: below)
    const int64_t base = (int64_t)blockIdx.x * LN_M;
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
#define LN_STAMP(k) do { if (a.stamps && tid == 0) a.stamps[(size_t)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
    LN_STAMP(0);
    int64_t tsrc = 0;                                        // DISTILL: the target row of the lane's sample of the loss phase
    uint2 tq[DISTILL ? 8 : 1];
    if constexpr (DISTILL) {
        if (wave < LN_GT) {
            int64_t j = base + 32 * wave + r < a.B ? base + 32 * wave + r : a.B - 1;
            tsrc = a.index ? a.index[j] : j;
        }
    }
    for (u32 k = threadIdx.x; k < 580; k += TK_BLOCK)
        bias_s[k] = k < 256 ? a.b1[k] : k < 512 ? a.b2[k - 256] : k < 576 ? a.b3[k - 512] : reinterpret_cast<const float *>(a.stats)[k - 576];
    // ---- gather: feature words and records of the tile's samples
    if (tid < LN_M) {
        int64_t j = base + tid < a.B ? base + tid : a.B - 1;
        int64_t src = a.index ? a.index[j] : j;
        const ulonglong2 *wp = reinterpret_cast<const ulonglong2 *>(a.words + src * 4);
        ulonglong2 w0 = wp[0], w1 = wp[1];
        ext[tid][0] = w0.x; ext[tid][1] = w0.y; ext[tid][2] = w1.x; ext[tid][3] = w1.y;
        if (base + tid < a.B) { a.Xw[(base + tid) * 2] = w0; a.Xw[(base + tid) * 2 + 1] = w1; }
        float4 rc = a.rec[src];
        if (base + tid >= a.B) rc.w = __uint_as_float(__float_as_uint(rc.w) & 0xFFu);       // (padding rows: weight 0)
        recs[tid] = rc;
    }
    if constexpr (DISTILL) {
        if (wave < LN_GT) {
            const uint2 *trow = a.target + tsrc * 16 + h;
#pragma unroll
            for (int k = 0; k < 8; k++) tq[k] = trow[2 * k];              // columns 32 ft + 8 q + 4 h .. + 3 at k = 4 ft + q
        }
    }
    __syncthreads();
    if (tid < 2 * LN_M) {   // expansion to bf16 0.0 / 1.0 (policy_expand, restated): two threads per sample, odd / even bytes
        u32 gme = tid >> 1, par = tid & 1;
        const uint4 *row = reinterpret_cast<const uint4 *>(&ext[gme][0]);
        uint4 r0 = row[0], r1 = row[1];
        u32 wd[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            u32 chunk = 2 * j + par;
            u32 byte = (wd[j >> 1] >> (8 * ((2 * (j & 1)) + par))) & 255u;
            *reinterpret_cast<uint4 *>(X + gme * PM_LD + 8 * chunk) = tk_expand_byte(byte);
        }
    }
    __syncthreads();
    LN_STAMP(1);
    f32x16 acc[2][LN_GT];
    // ---- layers 1 and 2: H = relu(W X + b), in place; layer 1 also leaves its ReLU mask
    // WHERE THE TILES ARE STORED.  On gfx9 one counter (vmcnt) counts a wave's loads and stores together, in order: a weight
    // fragment requested behind a tile's twelve stores is waited for behind their write acknowledgements, and with a tile
    // store between every two layers that wait was a quarter of the kernel (k_learn_chain without its stores: 298 -> 221 us).
    // So a tile leaves INSIDE the layer that follows it — that layer reads the same LDS tile — in the k-step that has just
    // requested the layer's last weight fragments: every load the wave still waits for was issued before the stores, and
    // nothing behind them is a vector-memory load until the next layer's weights (the biases come from LDS).
    auto hidden = [&](const __bf16 *w, const float *bias, bool keep_mask, auto tail) __attribute__((always_inline)) {
        chain_gemm<16>(acc, X, PM_LD, w, wave, tail);
        __syncthreads();                                   // every wave has read its last X fragment
#pragma unroll
        for (int ft = 0; ft < 2; ft++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                u32 f0 = wave * 64 + 32 * ft + 8 * q + 4 * h;
                float4 bv = *reinterpret_cast<const float4 *>(bias + f0);
#pragma unroll
                for (int gt = 0; gt < LN_GT; gt++) {
                    u32 o01 = ln_relu_bf16x2(acc[ft][gt][4 * q + 0], acc[ft][gt][4 * q + 1], bv.x, bv.y);
                    u32 o23 = ln_relu_bf16x2(acc[ft][gt][4 * q + 2], acc[ft][gt][4 * q + 3], bv.z, bv.w);
                    *reinterpret_cast<uint2 *>(X + (32 * gt + r) * PM_LD + f0) = make_uint2(o01, o23);
                    if (keep_mask) {                       // bits 0 / 16 of each pair -> one nibble: bit j = output j is positive
                        u32 t = ln_nonzero_u16x2(o01) | (ln_nonzero_u16x2(o23) << 2);
                        mask1[f0 >> 2][32 * gt + r] = (uint8_t)((t | (t >> 15)) & 15u);
                    }
                }
            }
        __syncthreads();
    };
    hidden(a.w1, bias_s, true, ChainNoTail());
    LN_STAMP(2);
    hidden(a.w2, bias_s + 256, false, [&]() __attribute__((always_inline)) { chain_store_tile(X, a.H1, base, a.B, tid); });
    LN_STAMP(3);
    // ---- layer 3 (64 outputs: 54 card logits, value in column 54) for samples [32 wave, 32 wave + 32), and the loss
    // in its accumulators: lane (r, h) holds outputs 32 ft + 8 q + 4 h + j of sample 32 wave + r, its partner lane ^ 32
    // the other half.  (Waves 0 .. LN_GT - 1: the fourth compute wave has no samples in this phase.)
    float s_pi = 0.f, s_v = 0.f, s_h = 0.f, s_w = 0.f, s_ce = 0.f, s_q = 0.f;
    if (wave < LN_GT) {
        const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16 *>(a.w3), 0, 2 * 16 * 1024, 0x00020000);
        auto wfrag = [&](int f) __attribute__((always_inline)) {
            return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, (int)(lane * 16), f * 1024, 0));
        };
        f32x16 o3[2];
#pragma unroll
        for (int ft = 0; ft < 2; ft++)
#pragma unroll
            for (int j = 0; j < 16; j++) o3[ft][j] = 0.f;
        bf16x8 wq[4][2];                                     // weight fragments four k-steps ahead (as in chain_gemm: an L2 round
#pragma unroll                                               // trip per k-step otherwise: this phase took 28k cycles of a 74k tile)
        for (int d = 0; d < 4; d++)
#pragma unroll
            for (int ft = 0; ft < 2; ft++) wq[d][ft] = wfrag(ft * 16 + d);
        bf16x8 xn = *reinterpret_cast<const bf16x8 *>(X + (32 * wave + r) * PM_LD + 8 * h);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < 16; kk++) {
            bf16x8 x = xn;
            bf16x8 wc[2] = {wq[kk & 3][0], wq[kk & 3][1]};
            if (kk + 4 < 16) {
#pragma unroll
                for (int ft = 0; ft < 2; ft++) wq[kk & 3][ft] = wfrag(ft * 16 + kk + 4);
            }
            if (kk < 15) xn = *reinterpret_cast<const bf16x8 *>(X + (32 * wave + r) * PM_LD + 16 * (kk + 1) + 8 * h);
            if (kk == 12) chain_store_tile(X, a.H2, base, a.B, tid);      // (the last weight fragments are on their way: as in chain_gemm)
#pragma unroll
            for (int ft = 0; ft < 2; ft++) o3[ft] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc[ft], x, o3[ft], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        const u32 gi = 32 * wave + r;
        const float4 rc = recs[gi];
        const float4 st = *reinterpret_cast<const float4 *>(bias_s + 576);
        u64 m = ext[gi][1] & TAROK_OBS_MASK;                 // feature word 1 = the legal cards
        u32 meta = __float_as_uint(rc.w);
        float w = (meta & 256u) ? 1.f : 0.f;
        const bool has_card = m != 0;
        if (!m) { m = 1; w = 0.f; }                          // nothing to play: no contribution, finite arithmetic
        u32 act = meta & 255u;
        act = act < 54 ? act : 53u;
        // The lane's 32 outputs: l[k], k = 16 ft + 4 q + j <-> output o = 32 ft + 8 q + 4 h + j.  Its legality bits come out of the
        // legal-card word by a nibble compaction (for each ft the four nibbles at bits 8 q + 4 h of that half of the word),
        // and an illegal card's logit becomes -1e30 ONCE: from there on its exponential, its probability and every term of the
        // gradient are zero without another test (p log p = 0 * finite).
        float l[32];
        u32 legal;
        {
            u32 m0 = (u32)m >> (4 * h), m1 = (u32)(m >> 32) >> (4 * h);
            u32 x0 = m0 & 0x0F0F0F0Fu, x1 = m1 & 0x0F0F0F0Fu;
            u32 y0 = (x0 | (x0 >> 4)) & 0x00FF00FFu, y1 = (x1 | (x1 >> 4)) & 0x00FF00FFu;
            legal = ((y0 | (y0 >> 8)) & 0xFFFFu) | ((y1 | (y1 >> 8)) << 16);
        }
#pragma unroll
        for (int ft = 0; ft < 2; ft++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float4 bv = *reinterpret_cast<const float4 *>(bias_s + 512 + 32 * ft + 8 * q + 4 * h);
                float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int j = 0; j < 4; j++) l[16 * ft + 4 * q + j] = o3[ft][4 * q + j] + bb[j];
            }
        // output 54 (the value) is l[16 + 4 * 2 + 2] = l[26] of the h = 1 lane
        float v_mine = (h == 1) ? l[26] : 0.f;
        float value = v_mine + __shfl_xor(v_mine, 32);
        float mx = -3.0e38f;
#pragma unroll
        for (int k = 0; k < 32; k++) {
            l[k] = ((legal >> k) & 1) ? l[k] : -1.0e30f;
            mx = fmaxf(mx, l[k]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        // z = logit - max; e = exp(z); log p = z - log(sum): one exponential per output and no logarithm per output
        const u32 act_h = act - 4 * h;                       // output o is the played card <=> its constant part equals this
        float sum = 0.f, za = 0.f, p_[32];
#pragma unroll
        for (int k = 0; k < 32; k++) {
            float z = l[k] - mx;
            float e = __expf(z);
            l[k] = z;
            p_[k] = e;
            sum += e;
            za = (act_h == (u32)(32 * (k >> 4) + 8 * ((k >> 2) & 3) + (k & 3))) ? z : za;
        }
        sum += __shfl_xor(sum, 32);
        za += __shfl_xor(za, 32);                            // (one of the pair holds the played card, which is legal)
        float ls = __logf(sum), inv = 1.0f / sum;
        // (the entropy's sum is written out like the gradient below, "ONE ROUNDING SEQUENCE": H - p log p with the product
        // rounded, but one fma in k = 26 and 27, the forms k_learn_chain<false> has had)
        float H = 0.f;
#pragma unroll
        for (int k = 0; k < 32; k++) {
#pragma clang fp contract(off)
            float p = p_[k] * inv;
            float lp = l[k] - ls;                            // log p (finite where p = 0: p log p = 0)
            H = (k == 26 || k == 27) ? __builtin_fmaf(-p, lp, H) : H - p * lp;
            p_[k] = p;
            l[k] = lp;
        }
        H += __shfl_xor(H, 32);
        float la = za - ls;
        float ratio = __expf(la - rc.x);
        float A = (rc.y - rc.z - st.x) * st.y;
        float rcl = fminf(fmaxf(ratio, 1.0f - a.clip), 1.0f + a.clip);
        float s1 = ratio * A, s2 = rcl * A;
        bool first = s1 <= s2, inside = ratio > 1.0f - a.clip && ratio < 1.0f + a.clip;
        float g = (first || inside) ? -A * ratio : 0.f;
        float dv = value - rc.y;
        if (h == 0) { s_pi = w * (-fminf(s1, s2)); s_v = w * dv * dv; s_h = w * H; s_w = w; }
        // DISTILL: the lane's 32 target values in the order of l[] / p_[], 0 where the card is not legal (select), ce and S
        float tqf[DISTILL ? 32 : 1], S = 0.f;
        if constexpr (DISTILL) {
            const u32 legal_q = has_card ? legal : 0u;
            float ce = 0.f;
#pragma unroll
            for (int k = 0; k < 32; k++) {
                const u32 pair = (k & 2) ? tq[k >> 2].y : tq[k >> 2].x;
                const float qv = __uint_as_float((k & 1) ? (pair & 0xFFFF0000u) : (pair << 16));
                const float qk = ((legal_q >> k) & 1) ? qv : 0.f;
                tqf[k] = qk;
                S += qk;
                ce -= qk * l[k];
            }
            S += __shfl_xor(S, 32);
            ce += __shfl_xor(ce, 32);
            if (h == 0) { s_ce = w * ce; s_q = w * S; }
        }
        // d loss / d output (unscaled: k_learn_reduce divides by the sum of the weights) -> D[sample][output], bf16; the sample's
        // weight folded into the two coefficients
        // ONE ROUNDING SEQUENCE, WRITTEN OUT.  Both instantiations compute the three terms' part of an element by the same
        // float32 operations, so that tarok_learn_chain_distill at coefficient 0 gives tarok_learn_chain's bytes: no
        // contraction is left to the compiler here (it chose differently for <false> and <true> in the two columns beside
        // the value's select: DESIGN.md section 8.5).  e = (ew p) (log p + H) rounds twice; then
        //     every column but the two below:   fma(gw, t, e)
        //     k = 26 (outputs 50 | 54):         gw t + e, both products rounded
        //     k = 27 (outputs 51 | 55):         fma(ew p, log p + H, gw t)
        // — the forms k_learn_chain<false> has had since the term was added: a plain launch computes what it always did.
        // DISTILL: + cw y, y = fma(S, p, -q), as one more fma, taken only where cw != 0 and y != 0: at coefficient 0, in every
        // row of weight 0, in a row without a teacher (64 zeros) and in the column of an illegal card the element keeps its
        // bytes (x + 0 would turn a -0 into +0, and 0 x a non-finite target is a NaN).
        const float gw = g * w, ew = a.ent_coef * w, dval = w * a.vf_coef * 2.0f * dv;
        float cw = 0.f;
        if constexpr (DISTILL) cw = a.distill_coef * w;
#pragma unroll
        for (int ft = 0; ft < 2; ft++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float d4[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
#pragma clang fp contract(off)
                    int k = 16 * ft + 4 * q + j;
                    float p = p_[k];
                    float t = (act_h == (u32)(32 * ft + 8 * q + j)) ? 1.0f - p : -p;
                    const float ep = ew * p, lh = l[k] + H;
                    if (k == 26) d4[j] = gw * t + ep * lh;
                    else if (k == 27) d4[j] = __builtin_fmaf(ep, lh, gw * t);
                    else d4[j] = __builtin_fmaf(gw, t, ep * lh);
                    if constexpr (DISTILL) {
                        const float y = __builtin_fmaf(S, p, -tqf[k]);
                        d4[j] = (cw != 0.f && y != 0.f) ? __builtin_fmaf(cw, y, d4[j]) : d4[j];
                    }
                    if (ft == 1 && q == 2 && j == 2) d4[j] = (h == 1) ? dval : d4[j];      // output 54: the value
                }
                *reinterpret_cast<uint2 *>(D + gi * LN_LDD + 32 * ft + 8 * q + 4 * h) = make_uint2(ln_bf16x2_of(d4[0], d4[1]), ln_bf16x2_of(d4[2], d4[3]));
            }
    } else {
        chain_store_tile(X, a.H2, base, a.B, tid);           // (the wave without samples: its share of H2 leaves at once)
    }
    // block sums of the loss terms (fixed order)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s_pi += __shfl_xor(s_pi, o); s_v += __shfl_xor(s_v, o); s_h += __shfl_xor(s_h, o); s_w += __shfl_xor(s_w, o); }
    if constexpr (DISTILL) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { s_ce += __shfl_xor(s_ce, o); s_q += __shfl_xor(s_q, o); }
        if (lane == 0) { red[4][wave] = s_ce; red[5][wave] = s_q; }
    }
    if (lane == 0) { red[0][wave] = s_pi; red[1][wave] = s_v; red[2][wave] = s_h; red[3][wave] = s_w; }
    __syncthreads();                                         // D complete; every wave is done with X (= H2) as an operand
    LN_STAMP(4);
    // ---- dH2 = (dOut W3) . (H2 > 0): K = 64; the mask is read off X (= H2) by the lane that overwrites it.  dOut leaves behind
    // the layer's (four k-steps of) weight loads
    chain_gemm<4>(acc, D, LN_LDD, a.w3t, wave, [&]() __attribute__((always_inline)) {
        __amdgpu_buffer_rsrc_t rs = chain_rows(reinterpret_cast<uint4 *>(a.dOut) + base * 8, base, a.B, 128);
#pragma unroll
        for (int it = 0; it < LN_M * 8 / TK_BLOCK; it++) {   // dOut tile -> global: LN_M rows of 128 bytes
            u32 piece = it * TK_BLOCK + tid, s_ = piece >> 3, c = piece & 7;
            chain_store16(rs, piece * 16, *reinterpret_cast<const uint4 *>(D + s_ * LN_LDD + 8 * c));
        }
    });
#pragma unroll
    for (int ft = 0; ft < 2; ft++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            u32 f0 = wave * 64 + 32 * ft + 8 * q + 4 * h;
#pragma unroll
            for (int gt = 0; gt < LN_GT; gt++) {
                uint2 *px = reinterpret_cast<uint2 *>(X + (32 * gt + r) * PM_LD + f0);
                uint2 hv = *px;                             // H2 >= 0: positive = non-zero; (0 / 1 per half) x 0xFFFF = the pair's AND mask
                u32 m01 = __umul24(ln_nonzero_u16x2(hv.x), 0xFFFFu), m23 = __umul24(ln_nonzero_u16x2(hv.y), 0xFFFFu);
                *px = make_uint2(ln_bf16x2_of(acc[ft][gt][4 * q + 0], acc[ft][gt][4 * q + 1]) & m01,
                                 ln_bf16x2_of(acc[ft][gt][4 * q + 2], acc[ft][gt][4 * q + 3]) & m23);
            }
        }
    __syncthreads();
    LN_STAMP(5);
    // ---- dH1 = (dH2 W2) . (H1 > 0); dH2 leaves inside
    chain_gemm<16>(acc, X, PM_LD, a.w2t, wave, [&]() __attribute__((always_inline)) { chain_store_tile(X, a.dH2, base, a.B, tid); });
    __syncthreads();
#pragma unroll
    for (int ft = 0; ft < 2; ft++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            u32 f0 = wave * 64 + 32 * ft + 8 * q + 4 * h;
#pragma unroll
            for (int gt = 0; gt < LN_GT; gt++) {
                u32 mk = mask1[f0 >> 2][32 * gt + r];
                *reinterpret_cast<uint2 *>(X + (32 * gt + r) * PM_LD + f0) =
                    make_uint2(ln_bf16x2_of(acc[ft][gt][4 * q + 0], acc[ft][gt][4 * q + 1]) & ln_pair_mask(mk & 3u),
                               ln_bf16x2_of(acc[ft][gt][4 * q + 2], acc[ft][gt][4 * q + 3]) & ln_pair_mask(mk >> 2));
            }
        }
    __syncthreads();
    chain_store_tile(X, a.dH1, base, a.B, tid);
    if (tid == 0) {                                          // block sums of the loss terms (here: not a store in front of a layer's loads)
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int k = 0; k < TK_BLOCK / 64; k++) { a0 += red[0][k]; a1 += red[1][k]; a2 += red[2][k]; a3 += red[3][k]; }
        a.part[blockIdx.x] = make_float4(a0, a1, a2, a3);
        if constexpr (DISTILL) {
            float c0 = 0.f, c1 = 0.f;
            for (int k = 0; k < TK_BLOCK / 64; k++) { c0 += red[4][k]; c1 += red[5][k]; }
            a.dpart[blockIdx.x] = make_float2(c0, c1);
        }
    }
    LN_STAMP(6);
#undef LN_STAMP
}

// ---------------------------------------------------------------------------------------------------------------
// Weight gradients.  For one layer: dW[o][i] = sum_s dH[s][o] * H[s][i] over the workgroup's chunk of samples, as
// D[i][o] = H^T dH with v_mfma_f32_32x32x16_bf16: A = H^T (row = input feature i), B = dH (column = output o),
// both k-contiguous along the SAMPLES — the transposed read of the row-major [sample][feature] tiles staged in LDS
// (ds_read_b64_tr_b16: per 16-lane group a block of 4 rows x 16 columns comes back column major).  The LDS row stride
// is 576 B (= 16 banks of 64): the two 4-row blocks a 32-lane half reads fall into disjoint banks.
// NB = 256: wave (wm, wn) owns inputs [128 wm, +128) x outputs [128 wn, +128): 4 x 4 tiles, 256 accumulator
// registers.  NB = 64 (layer 3, dH = dOut): wave w owns inputs [64 w, +64) x the 64 outputs: 2 x 2 tiles.
// WORDS: the H operand is the network input, expanded on the fly from the minibatch's feature words (layer 1; in
// minibatch order, as k_learn_chain wrote them: no index, no dependent load).
// Bias gradient: thread t sums column t of the staged dH tile.
#define DW_KT 32                    // samples per staged tile (k-steps of 16)
#define DW_ST 4                     // register stages: tiles in flight behind the one being computed
template <class F, int... I> __device__ __forceinline__ void static_for_impl(F &f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> __device__ __forceinline__ void static_for(F &&f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }
#define DW_LD 288                   // LDS row stride, bf16 elements
typedef __attribute__((ext_vector_type(4))) short s16x4;
__device__ __forceinline__ bf16x8 dw_frag(const __bf16 *tile, u32 k0, u32 f0) {
    u32 l = __lane_id(), g = l >> 4, q = (l >> 2) & 3, p = l & 3;
    const __bf16 *ad = tile + (k0 + (g >> 1) * 8 + q) * DW_LD + f0 + (g & 1) * 16 + 4 * p;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)ad);
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(ad + 4 * DW_LD));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

template <int NB, bool WORDS>
__device__ __forceinline__ void dw_layer(__bf16 *__restrict__ lds, int64_t s_begin, int64_t s_end, const uint4 *__restrict__ Hsrc,
                                         const u64 *__restrict__ words, const uint4 *__restrict__ dHsrc,
                                         float *__restrict__ outW, float *__restrict__ outB) {
    constexpr int TI = NB == 256 ? 4 : 2, TJ = NB == 256 ? 4 : 2;
    constexpr int PA = DW_KT * 32 / TK_BLOCK;               // 16-byte pieces of an H tile per thread (8)
    constexpr int PB = DW_KT * (NB / 8) / TK_BLOCK;         // ... of a dH tile (8, NB = 64: 2)
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const u32 ibase = NB == 256 ? 128 * (wave >> 1) : 64 * wave, obase = NB == 256 ? 128 * (wave & 1) : 0;
    // LDS tiles by OFFSET from the __shared__ array: through an array of pointers the compiler loses the address
    // space and emits flat loads / stores (which also wait for every global load in flight)
    auto offA = [](int b) { return (u32)(2 * b) * DW_KT * DW_LD; };
    auto offB = [](int b) { return (u32)(2 * b + 1) * DW_KT * DW_LD; };
    f32x16 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < TJ; j++)
#pragma unroll
            for (int k = 0; k < 16; k++) acc[i][j][k] = 0.f;
    float bcol[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // bias gradient: the eight columns of this thread's dH pieces
    // DW_ST register stages of a DW_KT-sample tile each: tile t is computed from LDS while the loads of tiles t + 2 ..
    // t + DW_ST + 1 are in flight (one workgroup per CU — 256 accumulator registers — so the bytes in flight per CU
    // are what hides the memory latency).  Per stage and thread: H rows as PA x 16 bytes (WORDS: 4 bytes of feature
    // bits per 32 samples), dH rows PB x 16.
    const int64_t ntiles = (s_end - s_begin + DW_KT - 1) / DW_KT;
    uint4 ra[DW_ST][PA], rb[DW_ST][PB];
    u32 rw[DW_ST][DW_KT / 32];
    const __amdgpu_buffer_rsrc_t rsA = WORDS ? __builtin_amdgcn_make_buffer_rsrc(const_cast<u64 *>(words), 0, (int)(s_end * 32), 0x00020000)
                                             : __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4 *>(Hsrc), 0, (int)(s_end * 512), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4 *>(dHsrc), 0, (int)(s_end * (NB * 2)), 0x00020000);
    auto tile_s0 = [&](int64_t t) { return s_begin + t * DW_KT; };
    auto fetch = [&](auto st, int64_t s0) __attribute__((always_inline)) {
        constexpr int S = decltype(st)::value;
        // (every load is issued whatever the row — a load under a branch would leave the compiler without a static
        // count of loads in flight, and every wait in the loop would become vmcnt(0).  BUFFER loads: the arrays as raw
        // buffers that END at the chunk's last row, so rows past it come back as zeros from the bounds check of the
        // instruction and nothing is tested or masked when a tile is staged; the tile's first row in the scalar offset,
        // one thread offset for all of a tile's loads.  Non-temporal: read once.)
        if (WORDS) {                                         // (words: the minibatch's feature words in minibatch order,
#pragma unroll                                               //  written by k_learn_chain: no index, no dependent load)
            for (int k = 0; k < DW_KT / 32; k++) rw[S][k] = __builtin_amdgcn_raw_buffer_load_b32(rsA, (int)((32 * k * 8 + tid) * 4), (int)(s0 * 32), 2);
        } else {
#pragma unroll
            for (int k = 0; k < PA; k++) {
                ln_u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rsA, (int)((tid + TK_BLOCK * k) * 16), (int)(s0 * 512), 2);
                ra[S][k] = make_uint4(t.x, t.y, t.z, t.w);
            }
        }
#pragma unroll
        for (int k = 0; k < PB; k++) {
            ln_u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rsB, (int)((tid + TK_BLOCK * k) * 16), (int)(s0 * (NB * 2)), 2);
            rb[S][k] = make_uint4(t.x, t.y, t.z, t.w);
        }
    };
    // (s0: first sample of the staged tile: rows at or past the chunk's end become zeros)
    auto stage = [&](auto st, int b, int64_t s0) __attribute__((always_inline)) {
        constexpr int S = decltype(st)::value;
        __bf16 *bufA_b = lds + offA(b), *bufB_b = lds + offB(b);
        if (WORDS) {
#pragma unroll
            for (int k2 = 0; k2 < DW_KT / 32; k2++) {
                u32 row = (tid >> 3) + 32 * k2, c0 = (tid & 7) * 32;      // 32 feature bits -> 32 bf16 = four 16-byte pieces
                u32 bits = rw[S][k2];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    *reinterpret_cast<uint4 *>(bufA_b + row * DW_LD + c0 + 8 * k) = tk_expand_byte((bits >> (8 * k)) & 255u);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < PA; k++) {
                u32 piece = tid + TK_BLOCK * k;
                *reinterpret_cast<uint4 *>(bufA_b + (piece >> 5) * DW_LD + 8 * (piece & 31)) = ra[S][k];
            }
        }
#pragma unroll
        for (int k = 0; k < PB; k++) {
            u32 piece = tid + TK_BLOCK * k, row = piece / (NB / 8), c16 = piece % (NB / 8);
            uint4 v = rb[S][k];
            *reinterpret_cast<uint4 *>(bufB_b + row * DW_LD + 8 * c16) = v;
            // bias gradient: the column sums of dH, taken here from the registers (every piece of this thread lies
            // in the same eight columns: 256 * k is a multiple of the pieces per row)
            u32 wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                bcol[2 * j] += __uint_as_float(wv[j] << 16);
                bcol[2 * j + 1] += __uint_as_float(wv[j] & 0xFFFF0000u);
            }
        }
    };
    // one tile from LDS buffer t & 1; then tile t + 1 (register stage NEXT) goes to the other buffer and that stage
    // is refilled with tile t + 1 + DW_ST
    auto step = [&](auto next_stage, int64_t t) __attribute__((always_inline)) {
        if (t >= ntiles) return;
        const int b = (int)(t & 1);
        const __bf16 *A = lds + offA(b), *Bt = lds + offB(b);
#pragma unroll 2
        for (u32 ks = 0; ks < DW_KT / 16; ks++) {
            bf16x8 af[TI], bfr[TJ];
#pragma unroll
            for (int i = 0; i < TI; i++) af[i] = dw_frag(A, 16 * ks, ibase + 32 * i);
#pragma unroll
            for (int j = 0; j < TJ; j++) bfr[j] = dw_frag(Bt, 16 * ks, obase + 32 * j);
#pragma unroll
            for (int i = 0; i < TI; i++)
#pragma unroll
                for (int j = 0; j < TJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        stage(next_stage, b ^ 1, tile_s0(t + 1));         // (buffer b ^ 1 was last read before the previous barrier)
        __builtin_amdgcn_sched_barrier(0);                // (the refill reuses the registers just staged: no loads hoisted above)
        fetch(next_stage, tile_s0(t + 1 + DW_ST));
        __syncthreads();
    };
    typedef std::integral_constant<int, 0> S0;
    static_for<DW_ST>([&](auto u) __attribute__((always_inline)) { fetch(u, tile_s0(decltype(u)::value)); });
    stage(S0{}, 0, tile_s0(0));
    __builtin_amdgcn_sched_barrier(0);
    fetch(S0{}, tile_s0(DW_ST));
    __syncthreads();
    for (int64_t t = 0; t < ntiles; t += DW_ST)           // tile t + u + 1 waits in stage (u + 1) mod DW_ST
        static_for<DW_ST>([&](auto u) __attribute__((always_inline)) {
            constexpr int U = decltype(u)::value;
            step(std::integral_constant<int, (U + 1) % DW_ST>{}, t + U);
        });
    // (the prologue staged tile 0 and the last step staged a tile past the end: both added zeros or real rows exactly
    // once to bcol — every tile is staged once)
    // D[row = input i][col = output o] -> outW[o][i]: four consecutive inputs per register quad
    const u32 r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < TJ; j++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                u32 o = obase + 32 * j + r, ii = ibase + 32 * i + 8 * q + 4 * h;
                *reinterpret_cast<float4 *>(outW + (size_t)o * 256 + ii) =
                    make_float4(acc[i][j][4 * q + 0], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
            }
    // bias gradient: threads with the same piece column hold partial sums (rows modulo the row stride of the pieces)
    float *bs = reinterpret_cast<float *>(lds);                  // (the tiles are done with: the last step ended with a barrier)
    constexpr int GROUPS = TK_BLOCK / (NB / 8);                  // threads per column group: 8 (NB = 64: 32)
    u32 c16 = tid % (NB / 8), grp = tid / (NB / 8);
#pragma unroll
    for (int j = 0; j < 8; j++) bs[grp * NB + c16 * 8 + j] = bcol[j];
    __syncthreads();
    if (tid < NB) {
        float t = 0.f;
#pragma unroll 8
        for (int g = 0; g < GROUPS; g++) t += bs[g * NB + tid];
        outB[tid] = t;
    }
    __syncthreads();                                             // (a caller may reuse the LDS)
}

// chunk c of a layer with `chunks` chunks over B samples: [begin, end), multiples of DW_KT
__device__ __forceinline__ void dw_chunk(int64_t B, u32 chunks, u32 c, int64_t &s0, int64_t &s1) {
    int64_t per = ((B + chunks - 1) / chunks + DW_KT - 1) / DW_KT * DW_KT;
    s0 = per * c < B ? per * c : B;
    s1 = s0 + per < B ? s0 + per : B;
}

// partials: layer 2 chunks [c2][65792], then layer 1 [c1][65792], then layer 3 [c3][16448] (weights, then the bias)
__global__ __launch_bounds__(TK_BLOCK) void k_learn_dw(int64_t B, u32 c2, u32 c1, u32 c3, const u64 *__restrict__ words,
                                                      const uint4 *__restrict__ H1,
                                                      const uint4 *__restrict__ H2, const uint4 *__restrict__ dOut,
                                                      const uint4 *__restrict__ dH2, const uint4 *__restrict__ dH1,
                                                      float *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) __bf16 lds[4 * DW_KT * DW_LD];
    u32 b = blockIdx.x;
    int64_t s0, s1;
    if (b < c2) {
        dw_chunk(B, c2, b, s0, s1);
        float *out = partial + (size_t)b * 65792;
        dw_layer<256, false>(lds, s0, s1, H1, nullptr, dH2, out, out + 65536);
    } else if (b < c2 + c1) {
        dw_chunk(B, c1, b - c2, s0, s1);
        float *out = partial + (size_t)c2 * 65792 + (size_t)(b - c2) * 65792;
        dw_layer<256, true>(lds, s0, s1, nullptr, words, dH1, out, out + 65536);
    } else {
        dw_chunk(B, c3, b - c2 - c1, s0, s1);
        float *out = partial + (size_t)(c2 + c1) * 65792 + (size_t)(b - c2 - c1) * 16448;
        dw_layer<64, false>(lds, s0, s1, H2, nullptr, dOut, out, out + 16384);
    }
}

// loss terms of the minibatch from k_learn_chain's block sums: terms = {pi, v, H, 1 / max(sum w, 1)} (weighted means)
TK_KERNEL(TK_BLOCK, 64) void k_learn_terms(int blocks, const float4 *__restrict__ part, float4 *__restrict__ terms,
                                                         float4 *__restrict__ running /* or NULL: += the terms (epoch statistics) */) {
    TK_VGPR_TOP(64, 63);
    __shared__ double red[4][TK_BLOCK];
    part_column_sums<4>(blocks, part, red);
    if (threadIdx.x == 0) {
        double inv = 1.0 / (red[3][0] < 1.0 ? 1.0 : red[3][0]);
        float4 t = make_float4((float)(red[0][0] * inv), (float)(red[1][0] * inv), (float)(red[2][0] * inv), (float)inv);
        terms[0] = t;
        if (running) { float4 q = running[0]; running[0] = make_float4(q.x + t.x, q.y + t.y, q.z + t.z, q.w + 1.f); }
    }
}

// k_learn_terms for tarok_learn_chain_distill, in its place: the same four terms by the same arithmetic (the same bits) and,
// from the chain's second array of block sums, dout = {sum w ce, sum w S} / max(sum w, 1): one reducer, one launch
TK_KERNEL(TK_BLOCK, 64) void k_learn_terms_distill(int blocks, const float4 *__restrict__ part, const float2 *__restrict__ dpart,
                                                   float4 *__restrict__ terms, float4 *__restrict__ running /* or NULL */,
                                                   float2 *__restrict__ dout, float2 *__restrict__ drunning /* or NULL: += dout */) {
    TK_VGPR_TOP(64, 63);
    __shared__ double red[6][TK_BLOCK];
    part_column_sums<4, 2>(blocks, part, red, dpart);
    if (threadIdx.x == 0) {
        double inv = 1.0 / (red[3][0] < 1.0 ? 1.0 : red[3][0]);
        float4 t = make_float4((float)(red[0][0] * inv), (float)(red[1][0] * inv), (float)(red[2][0] * inv), (float)inv);
        terms[0] = t;
        if (running) { float4 q = running[0]; running[0] = make_float4(q.x + t.x, q.y + t.y, q.z + t.z, q.w + 1.f); }
        float2 d = make_float2((float)(red[4][0] * inv), (float)(red[5][0] * inv));
        dout[0] = d;
        if (drunning) { float2 q = drunning[0]; drunning[0] = make_float2(q.x + d.x, q.y + d.y); }
    }
}

// flat gradient g[p] = terms.w * sum over the layer's chunks of partial[chunk][.]  (p in the flat parameter order);
// eight chunks in flight per thread
TK_KERNEL(TK_BLOCK, 64) void k_learn_reduce(u32 c2, u32 c1, u32 c3, const float *__restrict__ partial,
                                                          const float4 *__restrict__ terms, float *__restrict__ grad) {
    TK_VGPR_TOP(64, 63);
    u32 p = blockIdx.x * TK_BLOCK + threadIdx.x;
    if (p >= LN_P) return;
    const float *src;
    u32 chunks, stride;
    if (p < LN_P_W2)      { src = partial + (size_t)c2 * 65792 + (p - LN_P_W1); chunks = c1; stride = 65792; }   // W1 | b1 are contiguous in both
    else if (p < LN_P_W3) { src = partial + (p - LN_P_W2); chunks = c2; stride = 65792; }
    else                  { src = partial + (size_t)(c2 + c1) * 65792 + (p - LN_P_W3); chunks = c3; stride = 16448; }
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    u32 c = 0;
    for (; c + 8 <= chunks; c += 8) {
#pragma unroll
        for (u32 k = 0; k < 8; k++) s[k] += src[(size_t)(c + k) * stride];
    }
    for (; c < chunks; c++) s[0] += src[(size_t)c * stride];
    grad[p] = (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))) * terms[0].w;
}

// Gradient-norm clip + Adam (torch.optim.Adam semantics: bias-corrected, eps outside the square root) on the flat
// vectors, then the kernels' copies of the weights: bf16 in MFMA fragment order — [rows / 32][k-step][half][32][8],
// the weight fragment of output tile t, k-step kk, lane (r, h) is 16 contiguous bytes — for W1, W2, W3 (forward)
// and for the transposes W3^T [256 x 64], W2^T [256 x 256] (backward chain).  Two launches: k_learn_gnorm (sums of
// squares per workgroup) and k_learn_adam (every workgroup adds the few hundred partial sums up in the same order,
// then updates its 1,024 parameters): as ONE workgroup this step took 222 us — 145 dependent rounds of loads per
// thread — against 490 us for the weight gradients of 393,216 samples.
#define LN_ADAM_BLOCK 1024
#define LN_ADAM_BLOCKS ((LN_P + LN_ADAM_BLOCK - 1) / LN_ADAM_BLOCK)
struct AdamArgs {
    float *param, *grad, *m, *v;                 // [LN_P]
    int *step;                                   // device counter (k_learn_gnorm increments it)
    float lr, beta1, beta2, eps, max_norm;       // max_norm <= 0: no clipping
    __bf16 *w1, *w2, *w3, *w3t, *w2t;            // fragment-order copies (any may be NULL)
    float *gnorm;                                // the gradient norm before clipping, or NULL
    float *sumsq;                                // [LN_ADAM_BLOCKS] scratch: k_learn_gnorm's partial sums
    int apply;                                   // 0: only (re)build the weight copies from param
};
// (also advances the step counter: k_learn_adam, the next launch, reads the new value in every workgroup)
TK_KERNEL(LN_ADAM_BLOCK, 64) void k_learn_gnorm(const float *__restrict__ grad, float *__restrict__ sumsq, int *__restrict__ step) {
    TK_VGPR_TOP(64, 63);
    __shared__ float red[LN_ADAM_BLOCK / 64];
    u32 p = blockIdx.x * LN_ADAM_BLOCK + threadIdx.x;
    float g = p < LN_P ? grad[p] : 0.f;
    float ss = g * g;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < LN_ADAM_BLOCK / 64; k++) t += red[k];
        sumsq[blockIdx.x] = t;
        if (blockIdx.x == 0) *step = *step + 1;
    }
}
__device__ __forceinline__ void frag_store(__bf16 *dst, u32 ksteps, u32 row, u32 k, float val) {
    // element (row, k) of a [rows][16 ksteps] matrix -> [row / 32][k / 16][(k / 8) & 1][row & 31][k & 7]
    dst[((((size_t)(row >> 5) * ksteps + (k >> 4)) * 2 + ((k >> 3) & 1)) * 32 + (row & 31)) * 8 + (k & 7)] = (__bf16)val;
}
TK_KERNEL(LN_ADAM_BLOCK, 64) void k_learn_adam(AdamArgs a) {
    TK_VGPR_TOP(64, 63);
    const u32 tid = threadIdx.x, p = blockIdx.x * LN_ADAM_BLOCK + tid;
    float sc = 1.f, b1c = 1.f, b2c = 1.f;
    if (a.apply) {
        float t = 0.f;
        for (int k = 0; k < LN_ADAM_BLOCKS; k++) t += a.sumsq[k];      // (every thread, the same order: one value everywhere)
        float norm = sqrtf(t);
        if (a.gnorm && p == 0) *a.gnorm = norm;
        sc = (a.max_norm > 0.f && norm > a.max_norm) ? a.max_norm / (norm + 1e-6f) : 1.0f;
        int st = *a.step;                                    // (already advanced by k_learn_gnorm)
        b1c = 1.f - powf(a.beta1, (float)st); b2c = 1.f - powf(a.beta2, (float)st);
    }
    if (p >= LN_P) return;
    float w = a.param[p];
    if (a.apply) {
        float g = a.grad[p] * sc;
        float m = a.beta1 * a.m[p] + (1.f - a.beta1) * g;
        float v = a.beta2 * a.v[p] + (1.f - a.beta2) * g * g;
        a.m[p] = m; a.v[p] = v;
        w -= a.lr * (m / b1c) / (sqrtf(v / b2c) + a.eps);
        a.param[p] = w;
    }
    if (p < LN_P_B1) {                                   // W1[o][i]
        if (a.w1) frag_store(a.w1, 16, p >> 8, p & 255, w);
    } else if (p >= LN_P_W2 && p < LN_P_B2) {            // W2[o][i]; W2^T[i][o]
        u32 e = p - LN_P_W2;
        if (a.w2) frag_store(a.w2, 16, e >> 8, e & 255, w);
        if (a.w2t) frag_store(a.w2t, 16, e & 255, e >> 8, w);
    } else if (p >= LN_P_W3 && p < LN_P_B3) {            // W3[c][f]; W3^T[f][c] (64 columns: 4 k-steps)
        u32 e = p - LN_P_W3;
        if (a.w3) frag_store(a.w3, 16, e >> 8, e & 255, w);
        if (a.w3t) frag_store(a.w3t, 4, e & 255, e >> 8, w);
    }
}
