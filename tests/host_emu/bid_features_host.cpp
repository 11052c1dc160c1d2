// bid_feature_words (tarok_amd/csrc/tarok_device.h), the input row of tarok_bid_values, run on the CPU: g++ with the gfx950
// builtins emulated, for tests/test_bid_features_host.py.
//   bid_features_host seed offset n episode out.bin
// Per game i: the device's own deal and, for every seat v, the four feature words of (hand of v, v): 16 u64 per game.  The
// program checks on its own that words 2 and 3 are zero and that word 0 is the hand and one seat bit.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s seed offset n episode out.bin\n", argv[0]); return 2; }
    u64 seed = strtoull(argv[1], 0, 10), offset = strtoull(argv[2], 0, 10);
    long n = atol(argv[3]);
    u32 episode = (u32)atol(argv[4]);
    FILE *f = fopen(argv[5], "wb");
    if (!f) return 3;
    for (long i = 0; i < n; i++) {
        u64 hd[4], tal;
        deal_thread(game_key(seed, offset + (u64)i, episode), hd[0], hd[1], hd[2], hd[3], tal);
        u64 rec[4][4];
        for (u32 v = 0; v < 4; v++) {
            bid_feature_words(hd[v], v, rec[v]);
            if (rec[v][2] || rec[v][3] || rec[v][0] != (hd[v] | (1ULL << (54 + v)))) {
                fprintf(stderr, "game %ld seat %u: word 0 is not the hand and the seat, or a reserved word is set\n", i, v);
                return 4;
            }
        }
        fwrite(rec, sizeof rec, 1, f);
    }
    fclose(f);
    return 0;
}
