// tarok_front_lines (include/tarok_env.h; DESIGN.md §8.16): the bid and exchange heads on the dealt-ahead games.  Included by
// tarok_env.hip behind the heads' kernels, whose forward (mlp_prefetch / mlp_hidden / mlp_head / policy_expand) and decision
// code (bid_feature_words, bid_round, exchange_feature_words, exchange_choice, exchange_select, apply_exchange) it calls unchanged.
//
// A call is up to five launches on one stream:
//   k_front_zero      the count in the scratch's header and the histogram: zero
//   k_front_select    one thread per slot: the lines to take (valid tag, mark != tag) compacted into the item list
//   k_front_bid       32 items a workgroup: deal, the bidding head's forward on the four hands, the round, setup_game, and
//                     the Bot's exchange unless the exchange head takes it; the line's packed words
//   k_front_exchange  16 items a workgroup: the exchange head's forward on the waiting game, apply_exchange; the packed words
//   k_front_mark      one thread per item: the mark, the count and the contract histogram
// The grids of the last three are sized for the capacity (TK_AHEAD lines a slot); a workgroup whose first item lies at or
// beyond the device-side count leaves at once, and every item index is tested against the count before it is used.
// An item is slot << 4 | line.  The order of the list comes from atomics and changes from call to call; nothing depends on
// it: a row of an MFMA tile is computed from its own column of X alone.
#define TK_FRONT_HEAD_BYTES 128                     // the scratch's header: the count (u64), padded to an L2 line
#define TK_FRONT_MARK(ln) ((ln)->pad[0])            // byte 44 of a line: the episode the line was fronted for
static_assert(offsetof(AuxLine, pad) == 44, "the front mark lies behind the twelve bytes of key and tag the play kernels read");

__device__ __forceinline__ bool front_line_valid(u32 ep, u32 nep, u32 b) { return nep - ep - 1u < (u32)TK_AHEAD && TK_LINE(nep) == b; }

// the count and the histogram start a call at zero (a kernel, not a memset: one kind of node in a captured call)
TK_KERNEL(64, 64) void k_front_zero(unsigned long long *__restrict__ count, unsigned long long *__restrict__ hist_out) {
    TK_VGPR_TOP(64, 63);
    if (threadIdx.x == 0) count[0] = 0;
    if (hist_out && threadIdx.x < 10) hist_out[threadIdx.x] = 0;
}

TK_KERNEL(TK_BLOCK, 64) void k_front_select(int64_t n, const Aux *aux, const Counters *__restrict__ cnt, unsigned long long *count,
                                           u64 *__restrict__ items, int64_t cap) {
    TK_VGPR_TOP(64, 63);
    __shared__ u32 wcount;
    __shared__ unsigned long long wbase;
    const int64_t i = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (threadIdx.x == 0) wcount = 0;
    __syncthreads();
    u32 take = 0;
    if (i < n) {
        const u32 ep = cnt[i].episode;
#pragma unroll
        for (u32 b = 0; b < TK_AHEAD; b++) {
            const AuxLine *ln = &aux[i].line[b];
            const u32 nep = ln->nep, mark = TK_FRONT_MARK(ln);
            take |= (u32)(front_line_valid(ep, nep, b) && mark != nep) << b;
        }
    }
    const u32 c = (u32)__popc(take);
    const u32 pos = c ? atomicAdd(&wcount, c) : 0u;
    __syncthreads();
    if (threadIdx.x == 0) wbase = wcount ? atomicAdd(count, (unsigned long long)wcount) : 0ULL;
    __syncthreads();
    int64_t at = (int64_t)wbase + pos;
#pragma unroll
    for (u32 b = 0; b < TK_AHEAD; b++)
        if ((take >> b) & 1u) {
            if (at < cap) items[at] = ((u64)i << 4) | b;
            at++;
        }
}

// 32 items a workgroup, row = 4 * local item + seat — k_bid_values' tile.  Threads below 32 deal their item's game (the
// line's key) into LDS; after the head two lanes per row write the row's twenty values — k_bid_values[_pass]' scale, clamp,
// rounding and zeros — as the [4][TK_BID_ROWS] block bid_round reads, behind the logits in the activation buffer; threads
// below 32 then play the round and write the line.
template <bool PASS>
__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_front_bid(
    int64_t n, Aux *aux, const unsigned long long *__restrict__ count, const u64 *__restrict__ items,
    const __bf16 *__restrict__ w1, const float *__restrict__ b1, const __bf16 *__restrict__ w2, const float *__restrict__ b2,
    const __bf16 *__restrict__ w3, const float *__restrict__ b3, float scale, int playouts, int margin, u32 contracts, u32 seats,
    const uint8_t *__restrict__ seat_sets, int defer) {
    TK_VGPR_TOP(256, 255);
    constexpr u32 ITEMS = PM_M / 4;
    static_assert(TK_BLOCK == 2 * PM_M && TK_BID_ROWS == 20, "two lanes per row, five pieces per row");
    static_assert((PM_M * PM_LL + ITEMS * 4 * TK_BID_ROWS) * 4 <= PM_M * PM_LD * 2, "logits and values side by side in X");
    __shared__ __attribute__((aligned(16))) __bf16 X[PM_M * PM_LD];
    __shared__ u64 ext[PM_M][4];
    __shared__ u64 hand[ITEMS][5];
    __shared__ u32 iset[ITEMS];
    const u64 total = *count, base = (u64)blockIdx.x * ITEMS;
    if (base >= total) return;
    const u32 tid = threadIdx.x, wave = tid >> 6;
    float *L = reinterpret_cast<float *>(X);
    int *S = reinterpret_cast<int *>(L + PM_M * PM_LL);
    bf16x8 wq[4][2];
    mlp_prefetch(wq, w1, wave * 2);                // lands while the deals run
    if (tid < ITEMS) {
        u64 h0 = 0, h1 = 0, h2 = 0, h3 = 0, tal = 0;
        u32 set = 0;
        if (base + tid < total) {
            const u64 item = items[base + tid];
            const int64_t j = (int64_t)(item >> 4);
            if (j < n) {
                deal_thread(aux[j].line[item & 15u].nkey, h0, h1, h2, h3, tal);
                set = seat_sets ? (u32)seat_sets[j] & 15u : seats;
            }
        }
        hand[tid][0] = h0; hand[tid][1] = h1; hand[tid][2] = h2; hand[tid][3] = h3; hand[tid][4] = tal;
        iset[tid] = set;
    }
    __syncthreads();
    if (tid < PM_M) bid_feature_words(hand[tid >> 2][tid & 3u], tid & 3u, ext[tid]);
    __syncthreads();
    policy_expand(X, ext, tid);
    __syncthreads();
    mlp_hidden(X, w1, b1, wq, wave);
    mlp_prefetch(wq, w2, wave * 2);
    mlp_hidden(X, w2, b2, wq, wave);
    mlp_head(X, L, w3, b3, wave, 0);
    __syncthreads();
    {
        const u32 row = tid >> 1, v = row & 3u, li = row >> 2;
        const bool live = ((iset[li] >> v) & 1u) && hand[li][v] != 0;
        const u32 rowmask = live ? (bid_row_mask(contracts) | (PASS ? 1u << TK_BID_PASS_ROW : 0u)) : 0u;
#pragma unroll
        for (u32 p = tid & 1u; p < TK_BID_ROWS / 4; p += 2) {
            const float4 y = *reinterpret_cast<const float4 *>(L + row * PM_LL + 4 * p);
            const float yy[4] = {y.x, y.y, y.z, y.w};
            int vl[4];
#pragma unroll
            for (u32 j = 0; j < 4; j++) {
                const bool keep = (rowmask >> (4 * p + j)) & 1u;
                vl[j] = keep ? (int)rintf(fminf(fmaxf(yy[j] * scale, -1073741824.f), 1073741824.f)) : 0;
            }
            *reinterpret_cast<int4 *>(S + row * TK_BID_ROWS + 4 * p) = make_int4(vl[0], vl[1], vl[2], vl[3]);
        }
    }
    __syncthreads();
    if (tid >= ITEMS || base + tid >= total) return;
    const u64 item = items[base + tid];
    const int64_t j = (int64_t)(item >> 4);
    if (j >= n) return;
    AuxLine *ln = &aux[j].line[item & 15u];
    const u64 key = ln->nkey;
    const u32 set = iset[tid];
    u32 c, d, k;
    if (PASS) bid_round(key, S + tid * (4 * TK_BID_ROWS), playouts, margin, contracts, set, BidPassBar{}, c, d, k);
    else bid_round(key, S + tid * (4 * TK_BID_ROWS), playouts, margin, contracts, set, c, d, k);
    Game g;
    setup_game(g, hand[tid][0], hand[tid][1], hand[tid][2], hand[tid][3], hand[tid][4], c, d, k);
    g.epar = TK_LINE(ln->nep); g.cprev = 0;
    if (g.phase == TK_PHASE_EXCHANGE && !(defer && ((set >> g.declarer) & 1u))) bot_exchange(g, key);
    ulonglong2 a, b;
    pack(g, a.x, a.y, b.x, b.y);
    ln->n01 = a; ln->n23 = b;
}

// 16 items a workgroup, row = 8 * local item + talon group — k_exchange_values' tile.  Threads below 16 fetch their item's
// waiting game: the line's own words behind k_front_bid (FROM_LINE), or the Bot's setup re-made from the key — the game
// deal_into_buffer set up, before its exchange.  An item takes part iff that game waits for the exchange with its declarer
// in the set; the others keep their line.
template <bool FROM_LINE>
__global__ __launch_bounds__(TK_BLOCK, 2) TK_VGPR_BUDGET(256) void k_front_exchange(
    int64_t n, int mix, Aux *aux, const unsigned long long *__restrict__ count, const u64 *__restrict__ items,
    const __bf16 *__restrict__ w1, const float *__restrict__ b1, const __bf16 *__restrict__ w2, const float *__restrict__ b2,
    const __bf16 *__restrict__ w3, const float *__restrict__ b3, u32 seats, const uint8_t *__restrict__ seat_sets) {
    TK_VGPR_TOP(256, 255);
    constexpr u32 ROWS = 8, ITEMS = PM_M / ROWS;
    static_assert(TK_BLOCK == 2 * PM_M && PM_M % ROWS == 0, "one tile");
    __shared__ __attribute__((aligned(16))) __bf16 X[PM_M * PM_LD];
    __shared__ u64 ext[PM_M][4];
    __shared__ u64 pk[ITEMS][4];
    __shared__ u32 part[ITEMS];
    const u64 total = *count, base = (u64)blockIdx.x * ITEMS;
    if (base >= total) return;
    const u32 tid = threadIdx.x, wave = tid >> 6;
    float *L = reinterpret_cast<float *>(X);
    bf16x8 wq[4][2];
    mlp_prefetch(wq, w1, wave * 2);
    if (tid < ITEMS) {
        u64 p0 = 0, p1 = 0, p2 = 0, p3 = 0;
        u32 in = 0;
        if (base + tid < total) {
            const u64 item = items[base + tid];
            const int64_t j = (int64_t)(item >> 4);
            if (j < n) {
                const AuxLine *ln = &aux[j].line[item & 15u];
                const u32 set = seat_sets ? (u32)seat_sets[j] & 15u : seats;
                Game g;
                if (FROM_LINE) {
                    const ulonglong2 a = ln->n01, b = ln->n23;
                    unpack(g, a.x, a.y, b.x, b.y);
                } else {
                    const u64 key = ln->nkey;
                    u64 h0, h1, h2, h3, tal;
                    deal_thread(key, h0, h1, h2, h3, tal);
                    u32 c, d, k;
                    sample_setup(key, mix, c, d, k);
                    setup_game(g, h0, h1, h2, h3, tal, c, d, k);
                    g.epar = TK_LINE(ln->nep); g.cprev = 0;
                }
                in = g.phase == TK_PHASE_EXCHANGE && ((set >> g.declarer) & 1u);
                pack(g, p0, p1, p2, p3);
            }
        }
        pk[tid][0] = p0; pk[tid][1] = p1; pk[tid][2] = p2; pk[tid][3] = p3;
        part[tid] = in;
    }
    __syncthreads();
    if (tid < PM_M) {
        const u32 li = tid / ROWS;
        u64 w[4] = {0, 0, 0, 0};
        if (part[li]) {
            Game gm;
            unpack(gm, pk[li][0], pk[li][1], pk[li][2], pk[li][3]);
            exchange_feature_words(gm, tid & (ROWS - 1), w);
        }
#pragma unroll
        for (u32 q = 0; q < 4; q++) ext[tid][q] = w[q];
    }
    __syncthreads();
    policy_expand(X, ext, tid);
    __syncthreads();
    mlp_hidden(X, w1, b1, wq, wave);
    mlp_prefetch(wq, w2, wave * 2);
    mlp_hidden(X, w2, b2, wq, wave);
    mlp_head(X, L, w3, b3, wave, 0);
    __syncthreads();
    if (tid >= ITEMS || base + tid >= total || !part[tid]) return;
    const u64 item = items[base + tid];
    const int64_t j = (int64_t)(item >> 4);
    if (j >= n) return;
    Game g;
    unpack(g, pk[tid][0], pk[tid][1], pk[tid][2], pk[tid][3]);
    const u32 gs = group_size(g.contract), ngroups = 6u / gs;
    const float *y = L + tid * ROWS * PM_LL;
    const u32 ch = exchange_choice(y, PM_LL, ngroups);
    const u64 P = ext[tid * ROWS + ch][0] & TK_DECK;
    u64 cand = P & TK_DISCARDABLE;
    if ((u32)popc64(cand) < gs) cand = P;
    const u32 dpk = exchange_select(y + ch * PM_LL, cand, gs);
    apply_exchange(g, ch, dpk & 255u, (dpk >> 8) & 255u, (dpk >> 16) & 255u);
    ulonglong2 a, b;
    pack(g, a.x, a.y, b.x, b.y);
    AuxLine *ln = &aux[j].line[item & 15u];
    ln->n01 = a; ln->n23 = b;
}

// The mark of every item's line, the count and the contracts of the games fronted (hist_out zeroed by k_front_zero).
TK_KERNEL(TK_BLOCK, 64) void k_front_mark(int64_t n, Aux *aux, const unsigned long long *__restrict__ count, const u64 *__restrict__ items,
                                         int64_t *__restrict__ count_out, unsigned long long *__restrict__ hist_out) {
    TK_VGPR_TOP(64, 63);
    __shared__ u32 hist[10];
    const u64 total = *count, at = (u64)blockIdx.x * TK_BLOCK + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0 && count_out) count_out[0] = (int64_t)total;
    if ((u64)blockIdx.x * TK_BLOCK >= total) return;
    if (threadIdx.x < 10) hist[threadIdx.x] = 0;
    __syncthreads();
    if (at < total) {
        const u64 item = items[at];
        const int64_t j = (int64_t)(item >> 4);
        if (j < n) {
            AuxLine *ln = &aux[j].line[item & 15u];
            TK_FRONT_MARK(ln) = ln->nep;
            if (hist_out) {
                const ulonglong2 a = ln->n01, b = ln->n23;
                Game g;
                unpack(g, a.x, a.y, b.x, b.y);
                atomicAdd(&hist[g.contract < 10u ? g.contract : 9u], 1u);
            }
        }
    }
    __syncthreads();
    if (hist_out && threadIdx.x < 10 && hist[threadIdx.x]) atomicAdd(&hist_out[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

// tarok_get_lines: one thread per line; six words a line, and the line's game as tarok_get_state's ten lanes.
TK_KERNEL(TK_BLOCK, 64) void k_get_lines(int64_t n, const Aux *__restrict__ aux, u64 *__restrict__ lines_out, u64 *__restrict__ lanes_out) {
    TK_VGPR_TOP(64, 63);
    const int64_t t = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x, total = n * TK_AHEAD;
    if (t >= total) return;
    const AuxLine *ln = &aux[t / TK_AHEAD].line[t % TK_AHEAD];
    const ulonglong2 a = ln->n01, b = ln->n23;
    if (lines_out) {
        u64 *o = lines_out + t * 6;
        o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y; o[4] = ln->nkey; o[5] = (u64)ln->nep | ((u64)TK_FRONT_MARK(ln) << 32);
    }
    if (lanes_out) {
        Game g;
        unpack(g, a.x, a.y, b.x, b.y);
        state_lanes(g, [&](int lane, u64 v) { lanes_out[(int64_t)lane * total + t] = v; });
    }
}
