// The item numbering of tarok_playout_cards_net_sampled (tarok_amd/csrc/tarok_device.h: net_sampled_slots, net_sampled_slot,
// net_sampled_split, net_sampled_items) run on the CPU, g++, for tests/test_net_sampled_host.py.  A stand-alone program: for
// every (worlds, samples) in 1..8 x 1..8, and for the corners (64, 1024), (1, 1024) and (64, 1), it walks every slot, splits it
// and puts it together again, and marks it in a table: every slot is met once, in the order of ((j * worlds + w) * samples + k).
// It prints one line per shape — "worlds samples slots checksum", the checksum being the sum of (j + 13 w + 1031 k) * (slot + 1)
// over the slots —, then the item counts at the 2^31 border, then "ok <shapes>".
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <vector>

static int shape(u32 worlds, u32 samples) {
    const u32 slots = net_sampled_slots(worlds, samples);
    std::vector<unsigned char> met(slots, 0);
    unsigned long long sum = 0;
    u32 at = 0;
    for (u32 j = 0; j < 12; j++)
        for (u32 w = 0; w < worlds; w++)
            for (u32 k = 0; k < samples; k++, at++) {
                const u32 slot = net_sampled_slot(j, w, k, worlds, samples);
                if (slot != at || slot >= slots || met[slot]++) { printf("FAILED slot %u %u: %u %u %u\n", worlds, samples, j, w, k); return 1; }
                u32 j2, w2, k2;
                net_sampled_split(slot, worlds, samples, j2, w2, k2);
                if (j2 != j || w2 != w || k2 != k) { printf("FAILED split %u %u: %u\n", worlds, samples, slot); return 1; }
                sum += (unsigned long long)(j + 13u * w + 1031u * k) * (slot + 1u);
            }
    if (at != slots) { printf("FAILED count %u %u\n", worlds, samples); return 1; }
    printf("%u %u %u %llu\n", worlds, samples, slots, sum);
    return 0;
}

int main() {
    long shapes = 0;
    for (u32 worlds = 1; worlds <= 8; worlds++)
        for (u32 samples = 1; samples <= 8; samples++, shapes++)
            if (shape(worlds, samples)) return 1;
    const u32 corners[3][2] = {{64, 1024}, {1, 1024}, {64, 1}};
    for (int c = 0; c < 3; c++, shapes++)
        if (shape(corners[c][0], corners[c][1])) return 1;
    // 2^31 items are refused, one fewer is not: n = 2^20 games, 12 * 16 * 10 slots a game is under, 12 * 16 * 11 over
    printf("%lld %lld %lld %lld\n", (long long)net_sampled_items(1 << 20, 16, 10), (long long)net_sampled_items(1 << 20, 16, 11),
           (long long)net_sampled_items(2731, 64, 1024), (long long)net_sampled_items(2730, 64, 1024));
    printf("ok %ld\n", shapes);
    return 0;
}
