// The slot arithmetic of tarok_playout_cards_net_halving's compacted item list (tarok_amd/csrc/tarok_device.h:
// net_list_slot, net_list_count, net_list_alive, net_list_bound, net_list_tiles) run on the CPU, g++, for
// tests/test_net_halving_host.py.  A stand-alone program: exit status 0 and "ok <cases>" on stdout, or a line that names
// the first failure and status 1.
//   for every `on` word of 12 bits and W_r in {1, 2, 7, 16, 64}: walking (rank ascending, world ascending) the slots of a
//   game are base, base + 1, .. base + popc(on) * W_r - 1 — a bijection onto the game's range, in order —, and two games
//   laid one after the other by their counts do not overlap;
//   the alive bounds are 12, 6, 3, 2; the bound and the tiles are n * a_r * W_r and its ceiling in tiles.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int fail(const char *what, long a, long b, long c) {
    printf("FAILED %s %ld %ld %ld\n", what, a, b, c);
    return 1;
}

int main() {
    const u32 worlds[5] = {1, 2, 7, 16, 64};
    long cases = 0;
    for (u32 k = 0; k < 5; k++) {
        const u32 W = worlds[k];
        for (u32 on = 0; on < 4096; on++) {
            const u32 base = on * 37u + W;                        // any base: the slots are relative to it
            const u32 count = net_list_count(on, W);
            if (count != (u32)__builtin_popcount(on) * W) return fail("count", on, W, count);
            std::vector<unsigned char> hit(count, 0);             // sized to the game's range: a slot outside it is caught below
            u32 q = 0, next = base;
            for (u32 j = 0; j < 12; j++) {
                if (!((on >> j) & 1u)) continue;
                for (u32 lw = 0; lw < W; lw++) {
                    const u32 s = net_list_slot(base, q, W, lw);
                    if (s != next) return fail("order", on, W, s);
                    if (s < base || s - base >= count) return fail("range", on, W, s);
                    if (hit[s - base]++) return fail("twice", on, W, s);
                    next++;
                }
                q++;
            }
            for (u32 i = 0; i < count; i++)
                if (hit[i] != 1) return fail("hole", on, W, i);
            // the game after this one starts where this one ends
            if (net_list_slot(base + count, 0, W, 0) != next) return fail("next game", on, W, next);
            cases++;
        }
    }
    const u32 want[4] = {12, 6, 3, 2};
    for (u32 r = 0; r < 4; r++)
        if (net_list_alive(r) != want[r]) return fail("alive", r, net_list_alive(r), want[r]);
    for (u32 r = 0; r < 4; r++)
        for (u32 k = 0; k < 5; k++) {
            const int64_t n = 65536 + 17 * (int64_t)r, b = net_list_bound(n, r, worlds[k]);
            if (b != n * (int64_t)want[r] * (int64_t)worlds[k]) return fail("bound", r, worlds[k], (long)b);
            const int64_t t = net_list_tiles(b, 128);
            if (t * 128 < b || (t - 1) * 128 >= b) return fail("tiles", r, worlds[k], (long)t);
        }
    if (net_list_tiles(0, 128) != 0 || net_list_tiles(1, 128) != 1 || net_list_tiles(128, 128) != 1 || net_list_tiles(129, 128) != 2)
        return fail("tiles edge", 0, 0, 0);
    // the largest bound the launch accepts stays below 2^31 in the 64-bit arithmetic of the host
    if (net_list_bound((1LL << 31), 0, 64) != (1LL << 31) * 12 * 64) return fail("wide", 0, 0, 0);
    printf("ok %ld\n", cases);
    return 0;
}
