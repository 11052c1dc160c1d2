// The device side of tarok_playout_exchange (tarok_amd/csrc/tarok_device.h: exchange_discards, redeal_unseen on a game
// that waits for the exchange, apply_exchange on the world) run on the CPU, g++ with the gfx950 builtins emulated, for
// tests/test_exchange_host.py.
//   exchange_host seed offset n episode mix salt out.bin
// Every synthetic game is set up and left waiting for the exchange.  For a game that waits, candidate (i, d) = (w % ngroups,
// w) of world w = 0, 1: the helper's discards under the candidate key, and what the world looks like after redeal_unseen
// with the declarer as the viewer AND the candidate's exchange — the four hands, the four piles without the un-owned
// talon, the team, the seat whose pile bits hold the un-owned talon (255: none; 254: the cards disagree) — and the final
// scores of that game played out by the Bot under the world key (draw 128 + q), which go through score_game and so
// through the parking.  Record 0 also holds the helper's discards for group 0 under the GAME's key beside what
// bot_exchange does.  The program checks on its own that the re-deal touched only the pool's planes, the parked talon
// and the team, and that exchange-then-world gives the same game as world-then-exchange.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define WORLDS 2
#pragma pack(push, 1)
struct Rec {
    uint8_t waiting, declarer, gs, bot_same;
    uint8_t bot_disc[3], pad;
    uint8_t cand_i[WORLDS], cand_disc[WORLDS][3];
    u64 hands[WORLDS][4], piles[WORLDS][4];
    uint8_t team[WORLDS], park[WORLDS];
    int16_t scores[WORLDS][4];
};
#pragma pack(pop)

static u32 owner_of(const Game &g, u32 card) { return (u32)((g.A >> card) & 1) | ((u32)((g.B >> card) & 1) << 1); }
static u64 pile_rt(const Game &g, u32 s) { return g.C & seat_cards(g, s); }
static bool same_game(const Game &x, const Game &y) {
    return x.A == y.A && x.B == y.B && x.C == y.C && x.talon == y.talon && x.trick == y.trick && x.nt == y.nt && x.leader == y.leader &&
           x.trick_no == y.trick_no && x.phase == y.phase && x.contract == y.contract && x.declarer == y.declarer && x.king == y.king &&
           x.error == y.error && x.team == y.team && x.tl == y.tl;
}

int main(int argc, char **argv) {
    if (argc < 8) { fprintf(stderr, "usage: %s seed offset n episode mix salt out.bin\n", argv[0]); return 2; }
    u64 seed = strtoull(argv[1], 0, 10), offset = strtoull(argv[2], 0, 10);
    long n = atol(argv[3]);
    u32 episode = (u32)atol(argv[4]);
    int mix = atoi(argv[5]);
    u64 salt = strtoull(argv[6], 0, 10);
    FILE *f = fopen(argv[7], "wb");
    if (!f) return 3;
    for (long i = 0; i < n; i++) {
        u64 key = game_key(seed, offset + (u64)i, episode);
        u64 h0, h1, h2, h3, tal;
        deal_thread(key, h0, h1, h2, h3, tal);
        u32 c, d, k;
        sample_setup(key, mix, c, d, k);
        Game g;
        setup_game(g, h0, h1, h2, h3, tal, c, d, k);
        g.epar = 0; g.cprev = 0;
        Rec r;
        memset(&r, 0, sizeof r);
        if (g.phase == TK_PHASE_EXCHANGE) {
            const u32 gs = group_size(g.contract), ngroups = 6 / gs, decl = g.declarer;
            r.waiting = 1; r.declarer = (uint8_t)decl; r.gs = (uint8_t)gs;
            {   // group 0 under the game's own key: the Bot's exchange
                u32 dpk = exchange_discards(g, 0, key);
                for (int j = 0; j < 3; j++) r.bot_disc[j] = (uint8_t)(dpk >> (8 * j));
                Game x = g, y = g;
                bot_exchange(x, key);
                bool ok = apply_exchange(y, 0, dpk & 255, (dpk >> 8) & 255, (dpk >> 16) & 255);
                r.bot_same = ok && same_game(x, y);
            }
            const u64 pool = ~g.C & TK_DECK & ~hand_of(g, decl);
            for (u32 w = 0; w < WORLDS; w++) {
                const u32 ci = w % ngroups, cd = w;
                const u64 ebase = (u64)episode << 28;
                const u64 ckey = game_key(seed ^ salt, offset + (u64)i, (5ULL << 61) | ebase | ((u64)ci << 6) | (u64)cd);
                const u64 wkey = game_key(seed ^ salt, offset + (u64)i, (7ULL << 61) | ebase | (63ULL << 22) | (u64)w);
                const u32 dpk = exchange_discards(g, ci, ckey);
                r.cand_i[w] = (uint8_t)ci;
                for (int j = 0; j < 3; j++) r.cand_disc[w][j] = (uint8_t)(dpk >> (8 * j));
                Game x = g;
                redeal_unseen(x, decl, wkey);
                const u64 un0 = talon_unowned(x);
                if ((((x.A ^ g.A) | (x.B ^ g.B)) & ~(pool | un0)) || x.C != g.C || x.talon != g.talon || x.trick != g.trick || x.nt != g.nt ||
                    x.leader != g.leader || x.trick_no != g.trick_no || x.phase != g.phase || x.contract != g.contract ||
                    x.declarer != g.declarer || x.king != g.king || x.error != g.error || x.tl != g.tl || hand_of(x, decl) != hand_of(g, decl)) {
                    fprintf(stderr, "game %ld world %u: redeal_unseen touched more than the pool's planes, the parked talon and the team\n", i, w);
                    return 4;
                }
                if (!apply_exchange(x, ci, dpk & 255, (dpk >> 8) & 255, (dpk >> 16) & 255)) {
                    fprintf(stderr, "game %ld world %u: the candidate's exchange was rejected\n", i, w);
                    return 5;
                }
                Game y = g;                                              // the other order: exchange, then the world
                apply_exchange(y, ci, dpk & 255, (dpk >> 8) & 255, (dpk >> 16) & 255);
                redeal_unseen(y, decl, wkey);
                if (!same_game(x, y)) { fprintf(stderr, "game %ld world %u: exchange-then-world differs from world-then-exchange\n", i, w); return 6; }
                const u64 un = talon_unowned(x);
                for (u32 s = 0; s < 4; s++) { r.hands[w][s] = hand_of(x, s); r.piles[w][s] = pile_rt(x, s) & ~un; }
                r.team[w] = (uint8_t)x.team;
                u32 park = 255;
                for (u32 card = 0; card < 54; card++)
                    if ((un >> card) & 1) {
                        u32 o = owner_of(x, card);
                        park = (park == 255 || park == o) ? o : 254;
                    }
                r.park[w] = (uint8_t)park;
                u64 sc = 0; u32 ti = 0, q = 0;
                int fin = 0;
                while (!fin) { fin = apply_step<true>(x, policy_action(wkey, q, legal_now(x)), sc, ti, false); q++; }
                for (int s = 0; s < 4; s++) r.scores[w][s] = (int16_t)(sc >> (16 * s));
            }
        }
        fwrite(&r, sizeof r, 1, f);
    }
    fclose(f);
    return 0;
}
