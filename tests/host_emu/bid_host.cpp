// The device side of tarok_playout_bids and tarok_bid_round (tarok_amd/csrc/tarok_device.h: bid_world, bid_game, bid_answer,
// bid_round) run on the CPU, g++ with the gfx950 builtins emulated, for tests/test_bid_host.py.
//   bid_host seed offset n episode salt contracts threshold out.bin
// Per game i: the device's own deal; for every viewer v and world w = 0, 1 the world's four hands and talon ids under the
// world key, and the viewer's final score of ONE row, r = (i + 5 v + 11 w) % 19, played out as the kernel's item does
// (bid_game, the Bot's exchange under the playout key, the Bot's cards, draw 128 + q); then the bid round's three outputs
// on synthetic sums — sums[v][r] = rng32(key, 200 + 20 v + r) % 41 - 20, small so that ties happen — for the seat sets
// 0, 15 and 1 << (i & 3), with playouts = 1.  The program checks on its own that a world keeps the viewer's hand, the
// sizes 12 / 12 / 12 / 6 and the deck.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define WORLDS 2
#pragma pack(push, 1)
struct Rec {
    u64 hands[4][WORLDS][4], talon[4][WORLDS];
    int16_t score[4][WORLDS];
    int8_t bid[3][3];
    uint8_t pad[7];
};
#pragma pack(pop)

int main(int argc, char **argv) {
    if (argc < 9) { fprintf(stderr, "usage: %s seed offset n episode salt contracts threshold out.bin\n", argv[0]); return 2; }
    u64 seed = strtoull(argv[1], 0, 10), offset = strtoull(argv[2], 0, 10);
    long n = atol(argv[3]);
    u32 episode = (u32)atol(argv[4]);
    u64 salt = strtoull(argv[5], 0, 10);
    u32 contracts = (u32)atol(argv[6]);
    int threshold = atoi(argv[7]);
    FILE *f = fopen(argv[8], "wb");
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
                const u32 row = (u32)((i + 5 * v + 11 * w) % 19);
                Game h;
                bid_game(h, A, B, ids, row, v);
                u64 all = ids_mask(ids, 0, 6);
                for (u32 s = 0; s < 4; s++) {
                    r.hands[v][w][s] = hand_of(h, s);
                    if (popc64(r.hands[v][w][s]) != 12 || (all & r.hands[v][w][s])) { fprintf(stderr, "game %ld viewer %u world %u: hand sizes\n", i, v, w); return 4; }
                    all |= r.hands[v][w][s];
                }
                if (all != TK_DECK || popc64(ids_mask(ids, 0, 6)) != 6 || r.hands[v][w][v] != hd[v]) {
                    fprintf(stderr, "game %ld viewer %u world %u: the world lost the deck or the viewer's hand\n", i, v, w);
                    return 5;
                }
                r.talon[v][w] = ids;
                const u64 pkey = game_key(seed ^ salt, gidx, (3ULL << 61) | ebase | ((u64)v << 26) | ((u64)row << 21) | ((u64)w << 15));
                if (h.phase == TK_PHASE_EXCHANGE) bot_exchange(h, pkey);
                u64 sc = 0; u32 ti = 0, q = 0;
                int fin = 0;
                while (!fin) { fin = apply_step<true>(h, policy_action(pkey, q, legal_now(h)), sc, ti, false); q++; }
                r.score[v][w] = (int16_t)(sc >> (16 * v));
            }
        int32_t sums[4 * TK_BID_ROWS];
        for (u32 v = 0; v < 4; v++)
            for (u32 k = 0; k < TK_BID_ROWS; k++) sums[v * TK_BID_ROWS + k] = k < TK_BID_OPTIONS ? (int32_t)(rng32(key, 200 + 20 * v + k) % 41u) - 20 : 0;
        const u32 sets[3] = {0u, 15u, 1u << (i & 3)};
        for (int s = 0; s < 3; s++) {
            u32 c, d, k;
            bid_round(key, sets[s] ? sums : nullptr, 1, threshold, contracts, sets[s], c, d, k);
            r.bid[s][0] = (int8_t)c; r.bid[s][1] = (int8_t)d; r.bid[s][2] = (int8_t)k;
        }
        fwrite(&r, sizeof r, 1, f);
    }
    fclose(f);
    return 0;
}
