// halve_alive and best_alive (tarok_amd/csrc/tarok_device.h: the survivor rule and the final card of
// tarok_playout_cards_halving) run on the CPU, g++ with the gfx950 builtins emulated, for tests/test_halving_host.py.
//   halving_host seed n out.bin
// Per case: a [12][4] block of sums drawn from a small range (so that ties are common; every fourth case from a wide one),
// a random non-empty alive word and a seat; the record is the inputs and the two results.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>

struct Rec {
    int32_t row[48];
    uint32_t alive, seat, out, best;
};

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s seed n out.bin\n", argv[0]); return 2; }
    u64 s = strtoull(argv[1], 0, 10) * 0x9E3779B97F4A7C15ULL + 1;
    long n = atol(argv[2]);
    FILE *f = fopen(argv[3], "wb");
    if (!f) return 3;
    auto next = [&]() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (u32)(s >> 33); };
    for (long i = 0; i < n; i++) {
        Rec r;
        const int span = i % 4 == 3 ? 2000001 : 1 + (int)(next() % 5u);
        for (int k = 0; k < 48; k++) r.row[k] = (int)(next() % (u32)span) - span / 2;
        const u32 k = 1u + (u32)(i % 12);                       // k = 1 .. 12 alive ranks
        r.alive = 0;
        while ((u32)__builtin_popcount(r.alive) < k) r.alive |= 1u << (next() % 12u);
        r.seat = next() & 3u;
        r.out = halve_alive(r.row, r.alive, r.seat);
        r.best = best_alive(r.row, r.alive, r.seat);
        fwrite(&r, sizeof r, 1, f);
    }
    fclose(f);
    return 0;
}
