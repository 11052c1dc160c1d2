// The survivor rule, the bounds and the slot map of tarok_playout_exchange_net_halving / tarok_playout_bids_net_halving
// (tarok_amd/csrc/tarok_device.h: front_halving_keep, front_halving_stays, front_halving_alive, exchange_halving_bound,
// bid_halving_bound, front_halving_value, over net_list_slot / net_list_count) run on the CPU, g++, for
// tests/test_front_halving_host.py.  A stand-alone program: exit status 0 and "ok <cases>" on stdout, or a line that names the
// first failure and status 1.
//   the rule: for every alive count 1..48, random alive masks within 48 arms and random values with ties, the arms that
//   front_halving_stays keeps are the first `keep` of a stable sort by value descending (ties keep the lower index), and
//   their number is max(1, ceil(k / 2));
//   the bounds: a_r for a_0 in 1..48 against the recurrence, never below the alive count of a game halved r times;
//   the slot map: per round of a halved batch of units, (unit, alive bit, world) -> slot is an ascending bijection onto
//   [0, total) within B_r, for the exchange's six units a game and the bids' four with the pass bit;
//   the value: front_halving_value against the exact quotient where the count divides, and to the nearest elsewhere.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

static int fail(const char *what, long a, long b, long c) {
    printf("FAILED %s %ld %ld %ld\n", what, a, b, c);
    return 1;
}

static u64 rng_state = 0x9E3779B97F4A7C15ULL;
static u32 rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (u32)(rng_state >> 32);
}

// the arms of `alive` that stay, by the shared function, as a mask
static u64 stays_mask(const int *sums, u32 stride, u64 alive) {
    u64 out = 0;
    for (u32 j = 0; j < 64; j++)
        if (((alive >> j) & 1ULL) && front_halving_stays(sums, stride, alive, j)) out |= 1ULL << j;
    return out;
}

// the same by a stable sort
static u64 sorted_mask(const int *sums, u32 stride, u64 alive) {
    std::vector<u32> arms;
    for (u32 j = 0; j < 64; j++)
        if ((alive >> j) & 1ULL) arms.push_back(j);
    std::stable_sort(arms.begin(), arms.end(), [&](u32 a, u32 b) { return sums[a * stride] > sums[b * stride]; });
    const size_t k = arms.size(), keep = k > 1 ? (k + 1) / 2 : 1;
    u64 out = 0;
    for (size_t i = 0; i < keep && i < k; i++) out |= 1ULL << arms[i];
    return out;
}

// Lays the units' items by the prefix sum and walks them in (unit, bit, world) order: every slot once, ascending by one.
static int walk(const std::vector<u32> &on, u32 W, int64_t bound, const char *what, long a, long b) {
    std::vector<u32> base(on.size());
    u32 total = 0;
    for (size_t u = 0; u < on.size(); u++) { base[u] = total; total += net_list_count(on[u], W); }
    if ((int64_t)total > bound) return fail(what, a, b, total);
    std::vector<unsigned char> hit(total, 0);
    u32 next = 0;
    for (size_t u = 0; u < on.size(); u++)
        for (u32 r = 0; r < 32; r++) {
            if (!((on[u] >> r) & 1u)) continue;
            const u32 q = (u32)__builtin_popcount(on[u] & ((1u << r) - 1u));
            for (u32 w = 0; w < W; w++) {
                const u32 s = net_list_slot(base[u], q, W, w);
                if (s != next || s >= total || hit[s]++) return fail(what, a, b, s);
                next++;
            }
        }
    if (next != total) return fail(what, a, b, next);
    return 0;
}

int main() {
    long cases = 0;
    int sums[64 * 4];
    // the rule
    for (u32 k = 1; k <= 48; k++)
        for (u32 trial = 0; trial < 40; trial++) {
            u64 alive = 0;
            while ((u32)__builtin_popcountll(alive) < k) alive |= 1ULL << (rnd() % 48u);
            const u32 stride = 1u + (trial & 3u), span = trial < 8 ? 1u : (trial < 24 ? 3u : 1000u);     // few values: many ties
            for (u32 j = 0; j < 256; j++) sums[j] = 0;
            for (u32 j = 0; j < 48; j++) sums[j * stride] = (int)(rnd() % span) - (int)(span / 2);
            const u64 got = stays_mask(sums, stride, alive), want = sorted_mask(sums, stride, alive);
            if (got != want) return fail("rule", k, trial, (long)(got ^ want));
            if ((u32)__builtin_popcountll(got) != front_halving_keep(k) || front_halving_keep(k) != (k > 1 ? (k + 1) / 2 : 1))
                return fail("keep", k, trial, __builtin_popcountll(got));
            if (got & ~alive) return fail("outside alive", k, trial, 0);
            cases++;
        }
    {   // all equal: the lower indices stay
        for (u32 j = 0; j < 48; j++) sums[j] = 7;
        const u64 all = (1ULL << 48) - 1ULL;
        if (stays_mask(sums, 1, all) != (1ULL << 24) - 1ULL) return fail("stability", 48, 0, 0);
        if (stays_mask(sums, 1, 1ULL << 47) != 1ULL << 47) return fail("one arm", 47, 0, 0);
        cases++;
    }
    // the bounds
    for (u32 a0 = 1; a0 <= 48; a0++) {
        u32 a = a0;
        for (u32 r = 0; r < 4; r++) {
            if (front_halving_alive(a0, r) != a) return fail("alive", a0, r, a);
            a = (a + 1) / 2;
        }
        cases++;
    }
    if (exchange_halving_bound(65536, 4, 0, 2) != 65536LL * 24 * 2 || exchange_halving_bound(65536, 4, 3, 8) != 65536LL * 3 * 8)
        return fail("exchange bound", 0, 0, 0);
    if (bid_halving_bound(10, 15, false, 0xF, 1, 0, 2) != 10 * 4 * 14 * 2 || bid_halving_bound(10, 1, false, 0xF, 1, 2, 4) != 10 * 1 * 5 * 4 ||
        bid_halving_bound(10, 0, true, 1, 0, 3, 8) != 10 * 4 * 1 * 8)
        return fail("bid bound", 0, 0, 0);
    // the slot map, round after round of a halved batch
    for (u32 sets = 1; sets <= 8; sets++) {
        const u32 n = 14, ws[4] = {2, 1, 3, 5};
        std::vector<u64> alive(n);
        std::vector<u32> groups(n);
        for (u32 g = 0; g < n; g++) {
            groups[g] = g % 5 == 4 ? 0u : exchange_list_groups(1u + g % 6u);             // every fifth game does not take part
            alive[g] = groups[g] ? (1ULL << (groups[g] * sets)) - 1ULL : 0ULL;
        }
        for (u32 r = 0; r < 4; r++) {
            std::vector<u32> on;
            for (u32 g = 0; g < n; g++) {
                const bool plays = r == 0 || __builtin_popcountll(alive[g]) > 1;
                if ((u32)__builtin_popcountll(alive[g]) > front_halving_alive(6 * sets, r)) return fail("alive above a_r", sets, r, g);
                for (u32 i = 0; i < 6; i++) on.push_back(plays ? (u32)((alive[g] >> (i * sets)) & ((1u << sets) - 1u)) : 0u);
            }
            if (walk(on, ws[r], exchange_halving_bound(n, sets, r, ws[r]), "exchange slots", sets, r)) return 1;
            for (u32 g = 0; g < n; g++) {
                for (u32 j = 0; j < 48; j++) sums[j] = (int)(rnd() % 5u);
                if (alive[g]) alive[g] = stays_mask(sums, 1, alive[g]);
            }
            cases++;
        }
    }
    for (u32 contracts = 1; contracts <= 0x3FF; contracts += 7)
        for (u32 pass = 0; pass < 2; pass++) {
            const u32 n = 9, ws[4] = {1, 2, 2, 4}, rows = bid_row_mask(contracts);
            std::vector<u32> alive(n * 4), part(n * 4);
            for (u32 u = 0; u < n * 4; u++) { part[u] = (u * 7u + 3u) % 5u != 0u; alive[u] = part[u] ? rows : 0u; }
            for (u32 r = 0; r < 4; r++) {
                std::vector<u32> on;
                for (u32 u = 0; u < n * 4; u++) {
                    const bool plays = part[u] && (r == 0 || __builtin_popcount(alive[u]) > 1);
                    if ((u32)__builtin_popcount(alive[u]) > front_halving_alive((u32)__builtin_popcount(rows), r)) return fail("rows above a_r", contracts, r, u);
                    on.push_back(plays ? alive[u] | (pass ? 1u << 19 : 0u) : 0u);
                }
                if (walk(on, ws[r], bid_halving_bound(n, 0, true, contracts, pass, r, ws[r]), "bid slots", contracts, r)) return 1;
                for (u32 u = 0; u < n * 4; u++) {
                    for (u32 j = 0; j < 20; j++) sums[j] = (int)(rnd() % 3u);
                    if (alive[u]) alive[u] = (u32)stays_mask(sums, 1, alive[u]);
                }
                cases++;
            }
        }
    // the value
    for (int sum = -2000; sum <= 2000; sum += 37)
        for (int W = 1; W <= 64; W += 3)
            for (int c = 0; c <= W; c++) {
                const int v = front_halving_value(sum, W, c);
                if (c == 0) { if (v != 0) return fail("value at 0", sum, W, c); continue; }
                const long num = (long)sum * W;
                if (num % c == 0 && v != num / c) return fail("value exact", sum, W, c);
                const long d2 = 2 * ((long)v * c - num);                 // |v - num / c| <= 1/2
                if (d2 > c || d2 < -c) return fail("value nearest", sum, W, c);
                if ((d2 == c || d2 == -c) && ((num < 0) != (d2 < 0))) return fail("value half away from zero", sum, W, c);
            }
    cases++;
    printf("ok %ld\n", cases);
    return 0;
}
