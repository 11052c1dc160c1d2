// exchange_feature_words, exchange_choice and exchange_select (tarok_amd/csrc/tarok_device.h), the input rows and the
// decision of tarok_exchange_values, run on the CPU: g++ with the gfx950 builtins emulated, for
// tests/test_exchange_features_host.py.
//   exchange_features_host seed offset n episode out.bin
// Per game i and contract c = Tri .. Solo_ena (declarer (i + c) % 4, king (i / 4 + c) % 4): the device's own deal set up
// and left waiting for the exchange; the four feature words of rows 0..7; eight rows of 64 made-up network outputs —
// small integers, so that ties abound, with NaN, +inf and -inf sprinkled in —; the group exchange_choice picks and the
// discards exchange_select lays down from the winning row, on the candidates of the Bot's rule (every eighth game: on the
// whole hand, the mask of the rule's fallback).  The program checks on its own that rows at or beyond ngroups are zero
// and that the discards are distinct cards of the candidates.
#include <math.h>
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct Rec {
    u64 words[8][4];
    float y[8][64];
    u32 choice, dpk, cand_lo, cand_hi;
};

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s seed offset n episode out.bin\n", argv[0]); return 2; }
    u64 seed = strtoull(argv[1], 0, 10), offset = strtoull(argv[2], 0, 10);
    long n = atol(argv[3]);
    u32 episode = (u32)atol(argv[4]);
    FILE *f = fopen(argv[5], "wb");
    if (!f) return 3;
    for (long i = 0; i < n; i++) {
        u64 key = game_key(seed, offset + (u64)i, episode);
        u64 h0, h1, h2, h3, tal;
        deal_thread(key, h0, h1, h2, h3, tal);
        for (u32 c = TK_TRI; c <= TK_SOLO_ENA; c++) {
            Game g;
            setup_game(g, h0, h1, h2, h3, tal, c, (u32)((i + c) % 4), (u32)((i / 4 + c) % 4));
            g.epar = 0; g.cprev = 0;
            if (g.phase != TK_PHASE_EXCHANGE) { fprintf(stderr, "game %ld contract %u does not wait\n", i, c); return 4; }
            const u32 gs = group_size(c), ngroups = 6 / gs;
            Rec r;
            memset(&r, 0, sizeof r);
            for (u32 row = 0; row < 8; row++) {
                exchange_feature_words(g, row, r.words[row]);
                if (row >= ngroups && (r.words[row][0] | r.words[row][1] | r.words[row][2] | r.words[row][3])) {
                    fprintf(stderr, "game %ld contract %u row %u: a row the contract does not have is not zero\n", i, c, row);
                    return 5;
                }
                for (u32 o = 0; o < 64; o++) {
                    const u32 x = rng32(key, 1000 + 64 * (8 * c + row) + o);
                    float v = (float)((int)(x % 7u) - 3);
                    const u32 odd = (x >> 8) % 41u;
                    if (odd == 0) v = NAN;
                    if (odd == 1) v = INFINITY;
                    if (odd == 2) v = -INFINITY;
                    r.y[row][o] = v;
                }
            }
            r.choice = exchange_choice(&r.y[0][0], 64, ngroups);
            const u64 P = r.words[r.choice][0] & TK_DECK;
            u64 cand = P & TK_DISCARDABLE;
            if ((i & 7) == 7 || (u32)popc64(cand) < gs) cand = P;     // the fallback's mask, on every eighth game regardless
            r.cand_lo = (u32)cand; r.cand_hi = (u32)(cand >> 32);
            r.dpk = exchange_select(r.y[r.choice], cand, gs);
            u64 seen = 0;
            for (u32 j = 0; j < 3; j++) {
                const u32 d = (r.dpk >> (8 * j)) & 255u;
                if (j >= gs ? d != 255u : (d >= 54u || !((cand >> d) & 1ULL) || ((seen >> d) & 1ULL))) {
                    fprintf(stderr, "game %ld contract %u: discard %u is %u\n", i, c, j, d);
                    return 6;
                }
                if (j < gs) seen |= 1ULL << d;
            }
            fwrite(&r, sizeof r, 1, f);
        }
    }
    fclose(f);
    return 0;
}
