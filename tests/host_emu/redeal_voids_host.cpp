// redeal_voids (tarok_amd/csrc/tarok_device.h: the void-aware re-deal of the cards the seat to move cannot see, the
// world's team and the re-parking of the un-owned talon) run on the CPU, g++ with the gfx950 builtins emulated, for
// tests/test_redeal_voids_host.py.
//   redeal_voids_host seed offset n episode mix cards salt voids.bin out.bin
// voids.bin: [n][VARIANTS] u32, the void words to deal every game under (the test computes them from its model).
// Every synthetic game is played `cards` Bot cards on (or to its end); for a game still in play, every variant and
// worlds 0..3 the record holds what redeal_voids made of it: the four hands, the team, the seat whose pile bits hold the
// un-owned talon (255: there is none; 254: the cards disagree) and the final scores of the world played out by the Bot
// under the world key itself (draw 128 + q), which go through score_game and so through the parking.  The program
// checks on its own that nothing but the A/B planes of the pool and the team has changed.
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define WORLDS 4
#define VARIANTS 3
#pragma pack(push, 1)
struct Rec {
    uint8_t in_play, mover, played, pad[5];
    u64 hands[VARIANTS][WORLDS][4];
    uint8_t team[VARIANTS][WORLDS], park[VARIANTS][WORLDS];
    int16_t scores[VARIANTS][WORLDS][4];
};
#pragma pack(pop)

static u32 owner_of(const Game &g, u32 card) { return (u32)((g.A >> card) & 1) | ((u32)((g.B >> card) & 1) << 1); }

int main(int argc, char **argv) {
    if (argc < 10) { fprintf(stderr, "usage: %s seed offset n episode mix cards salt voids.bin out.bin\n", argv[0]); return 2; }
    u64 seed = strtoull(argv[1], 0, 10), offset = strtoull(argv[2], 0, 10);
    long n = atol(argv[3]);
    u32 episode = (u32)atol(argv[4]);
    int mix = atoi(argv[5]), cards = atoi(argv[6]);
    u64 salt = strtoull(argv[7], 0, 10);
    FILE *vf = fopen(argv[8], "rb");
    FILE *f = fopen(argv[9], "wb");
    if (!vf || !f) return 3;
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
        for (int t = 0; t < cards && g.phase == TK_PHASE_PLAY; t++) {
            u64 sc = 0; u32 ti = 0;
            apply_step<true>(g, policy_action(key, (u32)t, legal_now(g)), sc, ti, false);
        }
        Rec r;
        memset(&r, 0, sizeof r);
        u32 words[VARIANTS];
        if (fread(words, sizeof(u32), VARIANTS, vf) != VARIANTS) return 5;
        if (g.phase == TK_PHASE_PLAY) {
            u32 mover = (g.leader + g.nt) & 3, played = g.trick_no * 4 + g.nt;
            r.in_play = 1; r.mover = (uint8_t)mover; r.played = (uint8_t)played;
            u64 pool = ~g.C & TK_DECK & ~hand_of(g, mover);
            for (u32 v = 0; v < VARIANTS; v++)
            for (u32 w = 0; w < WORLDS; w++) {
                u64 wkey = game_key(seed ^ salt, offset + (u64)i, (7ULL << 61) | ((u64)episode << 28) | ((u64)played << 22) | (u64)w);
                Game x = g;
                redeal_voids(x, mover, wkey, words[v]);
                u64 un = talon_unowned(x);
                u64 moved = ((x.A ^ g.A) | (x.B ^ g.B)) & ~(pool | un);
                if (moved || x.C != g.C || x.talon != g.talon || x.trick != g.trick || x.nt != g.nt || x.leader != g.leader ||
                    x.trick_no != g.trick_no || x.phase != g.phase || x.contract != g.contract || x.declarer != g.declarer ||
                    x.king != g.king || x.error != g.error || x.tl != g.tl || x.epar != g.epar || x.cprev != g.cprev) {
                    fprintf(stderr, "game %ld world %u: redeal_voids touched more than the pool's planes and the team\n", i, w);
                    return 4;
                }
                for (u32 s = 0; s < 4; s++) r.hands[v][w][s] = hand_of(x, s);
                r.team[v][w] = (uint8_t)x.team;
                u32 park = 255;
                for (u32 card = 0; card < 54; card++)
                    if ((un >> card) & 1) {
                        u32 o = owner_of(x, card);
                        park = (park == 255 || park == o) ? o : 254;
                    }
                r.park[v][w] = (uint8_t)park;
                u64 sc = 0; u32 ti = 0, q = played;
                int fin = 0;
                while (!fin) { fin = apply_step<true>(x, policy_action(wkey, q, legal_now(x)), sc, ti, false); q++; }
                for (int s = 0; s < 4; s++) r.scores[v][w][s] = (int16_t)(sc >> (16 * s));
            }
        }
        fwrite(&r, sizeof r, 1, f);
    }
    fclose(f);
    fclose(vf);
    return 0;
}
