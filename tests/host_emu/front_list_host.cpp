// The `on` words and bounds of tarok_playout_exchange_net_list / tarok_playout_bids_net_list (tarok_amd/csrc/tarok_device.h:
// exchange_list_on, bid_list_on, exchange_list_bound, bid_list_bound, over net_list_slot / net_list_count) run on the CPU,
// g++, for tests/test_front_list_host.py.  A stand-alone program: exit status 0 and "ok <cases>" on stdout, or a line that
// names the first failure and status 1.
//   exchange: for every contract that has an exchange (1..6: three families of group sizes), sets 1..8, games in and out of
//   the seat set, W in {1, 3, 64}: over a batch of games the map (unit, row, world) -> slot, with base the exclusive prefix
//   sum of net_list_count over the units, is a bijection onto [0, total), ascends in (game, group, row, world) — which is the
//   dense launch's (g, r = i * sets + d, w) order —, and the total stays within exchange_list_bound;
//   bids: for every `contracts` value 1..0x3FF, both pass_value, every seat set (one launch-wide, and per-game sets with an
//   invalid deal row among the games), W in {1, 3}: the same, within bid_list_bound.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int fail(const char *what, long a, long b, long c) {
    printf("FAILED %s %ld %ld %ld\n", what, a, b, c);
    return 1;
}

// Lays the units' items by the prefix sum and walks them in (unit, row, world) order: every slot once, ascending by one.
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
            const u32 q = (u32)__builtin_popcount(on[u] & ((1u << r) - 1u));      // the sum kernels' rank of row r
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
    const u32 xw[3] = {1, 3, 64};
    for (u32 sets = 1; sets <= 8; sets++)
        for (u32 k = 0; k < 3; k++) {
            std::vector<u32> on;
            int64_t n = 0;
            for (u32 contract = 1; contract <= 6; contract++)
                for (u32 part = 0; part < 2; part++) {
                    const u32 groups = exchange_list_groups(contract), gs = group_size(contract);
                    if (groups * gs != 6) return fail("groups", contract, groups, gs);
                    for (u32 i = 0; i < 6; i++) {
                        const u32 o = exchange_list_on(contract, i, sets, part != 0);
                        if (o != ((part && i < groups) ? (1u << sets) - 1u : 0u)) return fail("exchange on", contract, i, o);
                        on.push_back(o);
                    }
                    n++;
                }
            if (walk(on, xw[k], exchange_list_bound(n, sets, xw[k]), "exchange", sets, xw[k])) return 1;
            cases++;
        }
    if (exchange_list_bound(65536, 4, 4) != 65536LL * 96) return fail("exchange bound", 0, 0, 0);
    for (u32 contracts = 1; contracts <= 0x3FF; contracts++)
        for (u32 pass = 0; pass < 2; pass++) {
            const u32 rows = bid_list_rows(contracts, pass);
            if ((rows & 0x7FFFFu) != bid_row_mask(contracts) || ((rows >> 19) & 1u) != pass || (rows >> 20)) return fail("rows", contracts, pass, rows);
            for (u32 r = 0; r < 19; r++)
                if (((rows >> r) & 1u) != ((contracts >> bid_row_contract(r)) & 1u)) return fail("row contract", contracts, r, rows);
            for (u32 W = 1; W <= 3; W += 2) {
                for (u32 seats = 0; seats < 16; seats++) {               // one launch-wide set: 3 games, the middle deal invalid
                    std::vector<u32> on;
                    for (u32 g = 0; g < 3; g++)
                        for (u32 v = 0; v < 4; v++) on.push_back(bid_list_on(contracts, pass, g != 1 && ((seats >> v) & 1u)));
                    if (walk(on, W, bid_list_bound(3, seats, false, contracts, pass, W), "bids", contracts, seats)) return 1;
                    cases++;
                }
                std::vector<u32> on;                                     // per-game sets: every set once
                for (u32 g = 0; g < 16; g++)
                    for (u32 v = 0; v < 4; v++) on.push_back(bid_list_on(contracts, pass, (g >> v) & 1u));
                if (walk(on, W, bid_list_bound(16, 0, true, contracts, pass, W), "bids per game", contracts, W)) return 1;
                cases++;
            }
        }
    // one viewer at the default contracts: 13 rows a game
    if (bid_list_bound(1, 1, false, 0xF, 0, 1) != 13 || bid_list_bound(1, 15, false, 0xF, 1, 2) != 4 * 14 * 2) return fail("bid bound", 0, 0, 0);
    if (bid_list_bound(1LL << 24, 15, false, 0x3FF, 1, 64) < (1LL << 31)) return fail("wide", 0, 0, 0);
    printf("ok %ld\n", cases);
    return 0;
}
