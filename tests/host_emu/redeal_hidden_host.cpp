// redeal_hidden (tarok_amd/csrc/tarok_device.h: the re-deal of the three other hands together with Klop's face-down talon
// or the declarer's discards) run on the CPU, g++ with the gfx950 builtins emulated, for tests/test_redeal_hidden_host.py.
//   redeal_hidden_host seed offset n episode mix cards salt out.bin
// Every synthetic game is played `cards` Bot cards on (or to its end), the word of played cards kept beside it; for a
// game still in play and worlds 0..1 the record holds what redeal_hidden made of it: the four hands, the four won piles
// (without the cards on the table and the un-owned talon), the talon ids, the team, the seat whose pile bits hold the
// un-owned talon (255: there is none; 254: the cards disagree) and the final scores of the world played out by the Bot
// under the world key itself (draw 128 + q), which go through score_game, the parking and Klop's gifts.  The program
// checks on its own that the fields a world must keep are kept and that no card is lost or doubled.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define WORLDS 2
#pragma pack(push, 1)
struct Rec {
    uint8_t in_play, mover, played, pad[5];
    u64 word;
    u64 hands[WORLDS][4], piles[WORLDS][4], talon[WORLDS];
    uint8_t team[WORLDS], park[WORLDS], pad2[4];
    int16_t scores[WORLDS][4];
};
#pragma pack(pop)

static u32 owner_of(const Game &g, u32 card) { return (u32)((g.A >> card) & 1) | ((u32)((g.B >> card) & 1) << 1); }

int main(int argc, char **argv) {
    if (argc < 9) { fprintf(stderr, "usage: %s seed offset n episode mix cards salt out.bin\n", argv[0]); return 2; }
    u64 seed = strtoull(argv[1], 0, 10), offset = strtoull(argv[2], 0, 10);
    long n = atol(argv[3]);
    u32 episode = (u32)atol(argv[4]);
    int mix = atoi(argv[5]), cards = atoi(argv[6]);
    u64 salt = strtoull(argv[7], 0, 10);
    FILE *f = fopen(argv[8], "wb");
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
        if (g.phase == TK_PHASE_EXCHANGE) bot_exchange(g, key);
        u64 word = 0;
        for (int t = 0; t < cards && g.phase == TK_PHASE_PLAY; t++) {
            u64 sc = 0; u32 ti = 0;
            u32 a = policy_action(key, (u32)t, legal_now(g));
            word |= 1ULL << a;
            apply_step<true>(g, a, sc, ti, false);
        }
        Rec r;
        memset(&r, 0, sizeof r);
        if (g.phase == TK_PHASE_PLAY) {
            u32 mover = (g.leader + g.nt) & 3, played = g.trick_no * 4 + g.nt;
            r.in_play = 1; r.mover = (uint8_t)mover; r.played = (uint8_t)played; r.word = word;
            u64 table = 0;
            for (u32 j = 0; j < g.nt; j++) table |= 1ULL << ((g.trick >> (6 * j)) & 63);
            for (u32 w = 0; w < WORLDS; w++) {
                u64 wkey = game_key(seed ^ salt, offset + (u64)i, (7ULL << 61) | ((u64)episode << 28) | ((u64)played << 22) | (u64)w);
                Game x = g;
                redeal_hidden(x, mover, wkey, word);
                if (hand_of(x, mover) != hand_of(g, mover) || (x.C & table) != table || x.trick != g.trick || x.nt != g.nt ||
                    x.leader != g.leader || x.trick_no != g.trick_no || x.phase != g.phase || x.contract != g.contract ||
                    x.declarer != g.declarer || x.king != g.king || x.error != g.error || x.tl != g.tl || x.epar != g.epar ||
                    x.cprev != g.cprev || (x.talon >> 36) != 0 || ((x.A | x.B | x.C) & ~TK_DECK) != 0) {
                    fprintf(stderr, "game %ld world %u: redeal_hidden touched what a world keeps\n", i, w);
                    return 4;
                }
                u64 un = talon_unowned(x);
                if (popc64(un) != popc64(talon_unowned(g)) || popc64(x.C) != popc64(g.C) || popc64(talon_all(x)) != 6) {
                    fprintf(stderr, "game %ld world %u: a card was lost or doubled\n", i, w);
                    return 5;
                }
                for (u32 s = 0; s < 4; s++) {
                    r.hands[w][s] = hand_of(x, s);
                    r.piles[w][s] = seat_cards(x, s) & x.C & ~un & ~table;
                }
                r.talon[w] = x.talon;
                r.team[w] = (uint8_t)x.team;
                u32 park = 255;
                for (u32 card = 0; card < 54; card++)
                    if ((un >> card) & 1) {
                        u32 o = owner_of(x, card);
                        park = (park == 255 || park == o) ? o : 254;
                    }
                r.park[w] = (uint8_t)park;
                u64 sc = 0; u32 ti = 0, q = played;
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
