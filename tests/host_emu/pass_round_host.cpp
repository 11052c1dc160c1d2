// The device side of tarok_playout_bids_pass and tarok_bid_round_pass (tarok_amd/csrc/tarok_device.h: pass_round,
// bid_game_as, pass_bar, the pass-aware bid_answer / bid_round) run on the CPU, g++ with the gfx950 builtins emulated, for
// tests/test_pass_round_host.py.
//   pass_round_host seed offset n episode salt contracts margin playouts out.bin
// Per game i: the device's own deal; for every viewer v and world w = 0, 1 the pass round's contract, declarer and king
// under the playout key of row 19 (sample k = i % 3) and the viewer's final score of the pass playout, played as the
// kernel's item plays it (bid_world, pass_round, bid_game_as, the Bot's exchange, the Bot's cards, draw 128 + q); then the
// pass-aware bid round's three outputs on synthetic sums — sums[v][r] = rng32(key, 200 + 20 v + r) % 41 - 20, row 19
// included — for the seat sets 0, 15 and 1 << (i & 3).  The program checks on its own that with row 19 zeroed the
// pass-aware round is bid_round at threshold = margin, and that the muted seat declares nothing but seat 0's forced Klop.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define WORLDS 2
#pragma pack(push, 1)
struct Rec {
    int8_t round[4][WORLDS][3];
    int16_t score[4][WORLDS];
    int8_t bid[3][3];
    uint8_t pad[7];
};
#pragma pack(pop)

int main(int argc, char **argv) {
    if (argc < 10) { fprintf(stderr, "usage: %s seed offset n episode salt contracts margin playouts out.bin\n", argv[0]); return 2; }
    u64 seed = strtoull(argv[1], 0, 10), offset = strtoull(argv[2], 0, 10);
    long n = atol(argv[3]);
    u32 episode = (u32)atol(argv[4]);
    u64 salt = strtoull(argv[5], 0, 10);
    u32 contracts = (u32)atol(argv[6]);
    int margin = atoi(argv[7]), playouts = atoi(argv[8]);
    FILE *f = fopen(argv[9], "wb");
    if (!f) return 3;
    for (long i = 0; i < n; i++) {
        const u64 gidx = offset + (u64)i, key = game_key(seed, gidx, episode), ebase = (u64)episode << 28;
        u64 hd[4], tal;
        deal_thread(key, hd[0], hd[1], hd[2], hd[3], tal);
        Rec r;
        memset(&r, 0, sizeof r);
        for (u32 v = 0; v < 4; v++)
            for (u32 w = 0; w < WORLDS; w++) {
                u64 A, B, ids;
                bid_world(hd[0], hd[1], hd[2], hd[3], tal, v, game_key(seed ^ salt, gidx, (2ULL << 61) | ebase | ((u64)v << 6) | (u64)w), A, B, ids);
                const u64 pkey = game_key(seed ^ salt, gidx, (3ULL << 61) | ebase | ((u64)v << 26) | ((u64)TK_BID_PASS_ROW << 21) |
                                                                 ((u64)w << 15) | (u64)(i % 3));
                u32 c, d, kg;
                pass_round(pkey, v, c, d, kg);
                if (d == v && !(v == 0 && c == TK_KLOP)) { fprintf(stderr, "game %ld viewer %u world %u: the muted seat declares\n", i, v, w); return 4; }
                r.round[v][w][0] = (int8_t)c; r.round[v][w][1] = (int8_t)d; r.round[v][w][2] = (int8_t)kg;
                Game h;
                bid_game_as(h, A, B, ids, c, d, kg);
                if (hand_of(h, v) != hd[v]) { fprintf(stderr, "game %ld viewer %u world %u: the viewer's hand\n", i, v, w); return 5; }
                if (h.phase == TK_PHASE_EXCHANGE) bot_exchange(h, pkey);
                u64 sc = 0; u32 ti = 0, q = 0;
                int fin = 0;
                while (!fin) { fin = apply_step<true>(h, policy_action(pkey, q, legal_now(h)), sc, ti, false); q++; }
                r.score[v][w] = (int16_t)(sc >> (16 * v));
            }
        int32_t sums[4 * TK_BID_ROWS], flat[4 * TK_BID_ROWS];
        for (u32 v = 0; v < 4; v++)
            for (u32 k = 0; k < TK_BID_ROWS; k++) {
                sums[v * TK_BID_ROWS + k] = (int32_t)(rng32(key, 200 + 20 * v + k) % 41u) - 20;
                flat[v * TK_BID_ROWS + k] = k == TK_BID_PASS_ROW ? 0 : sums[v * TK_BID_ROWS + k];
            }
        const u32 sets[3] = {0u, 15u, 1u << (i & 3)};
        for (int s = 0; s < 3; s++) {
            u32 c, d, k, c0, d0, k0, c1, d1, k1;
            bid_round(key, sets[s] ? sums : nullptr, playouts, margin, contracts, sets[s], BidPassBar{}, c, d, k);
            r.bid[s][0] = (int8_t)c; r.bid[s][1] = (int8_t)d; r.bid[s][2] = (int8_t)k;
            bid_round(key, sets[s] ? flat : nullptr, playouts, margin, contracts, sets[s], BidPassBar{}, c0, d0, k0);
            bid_round(key, sets[s] ? flat : nullptr, playouts, margin, contracts, sets[s], c1, d1, k1);
            if (c0 != c1 || d0 != d1 || k0 != k1) { fprintf(stderr, "game %ld set %u: row 19 zero is not bid_round at threshold = margin\n", i, sets[s]); return 6; }
        }
        if (pass_bar(-7, 3, 5) != 8 || pass_bar(2147483647, 2147483647, 2147483647) != 2147483647LL + 2147483647LL * 2147483647LL) return 7;
        fwrite(&r, sizeof r, 1, f);
    }
    fclose(f);
    return 0;
}
