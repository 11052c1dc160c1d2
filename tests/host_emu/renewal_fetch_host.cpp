// The words k_play_wide's trick-aligned card loop carries from card to card (tarok_amd/csrc/tarok_device.h: RngCtr /
// rng_ctr, obs_carry / obs_word_with on the carried word) run on the CPU, g++ with the gfx950 builtins emulated, for
// tests/test_renewal_fetch_host.py.
//   renewal_fetch_host rng                                  the premultiplied counter against rng32(key, 128 + pos)
//   renewal_fetch_host seed offset n episodes mix out.bin   `episodes` consecutive games per slot, played the way the loop
//                                                           plays them: both words advanced per card, reset on renewal
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>

static int rng_check() {
    u64 r = 0x2545F4914F6CDD1DULL;
    unsigned long long draws = 0;
    for (int it = 0; it < 4000; it++) {
        r ^= r << 13; r ^= r >> 7; r ^= r << 17;
        u64 key = it < 4 ? (it & 1 ? ~0ULL : 0ULL) ^ ((u64)(it >> 1) << 63) : r;
        RngCtr c = rng_ctr(128u);
        for (u32 pos = 0; pos < 48; pos++, draws++) {
            u32 want = rng32(key, 128u + pos);
            if (rng32(key, rng_ctr(128u + pos)) != want || rng32(key, c) != want || rng32((u32)key, (u32)(key >> 32), c) != want) {
                fprintf(stderr, "key %016llx pos %u: premultiplied counter draws another number\n", (unsigned long long)key, pos);
                return 1;
            }
            c.v += TK_RNG_STEP;
        }
    }
    printf("%llu draws\n", draws);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && argv[1][0] == 'r') return rng_check();
    if (argc < 7) { fprintf(stderr, "usage: %s rng | seed offset n episodes mix out.bin\n", argv[0]); return 2; }
    u64 seed = strtoull(argv[1], 0, 10), offset = strtoull(argv[2], 0, 10);
    long n = atol(argv[3]);
    int episodes = atoi(argv[4]);
    int mix = atoi(argv[5]);
    FILE *f = fopen(argv[6], "wb");
    if (!f) return 3;
    for (long i = 0; i < n; i++) {
        u32 rctr = 0, ocar = 0;                  // carried across the games of the slot, as the loop carries them
        for (int e = 0; e < episodes; e++) {
            u64 key = game_key(seed, offset + (u64)i, (u64)e);
            u64 h0, h1, h2, h3, tal;
            deal_thread(key, h0, h1, h2, h3, tal);
            u32 c, d, k;
            sample_setup(key, mix, c, d, k);
            Game g;
            setup_game(g, h0, h1, h2, h3, tal, c, d, k);
            g.epar = 0; g.cprev = 0;
            if (g.phase == TK_PHASE_EXCHANGE) bot_exchange(g, key);
            if (e == 0) {                        // before the loop (tricks())
                rctr = rng_ctr(128u + g.trick_no * 4).v;
                ocar = obs_carry(g.leader, g.trick_no << 2);
            } else {                             // what the renewal left: checked against the fresh game
                if (rctr != rng_ctr(128u).v || ocar != obs_carry(g.leader, 0)) { fprintf(stderr, "slot %ld game %d: words after renewal\n", i, e); return 4; }
            }
            uint8_t actions[48], half[48];
            int16_t played = 0;
            for (int t = 0; t < 48; t++) { actions[t] = 255; half[t] = 255; }
            for (int t = 0; t < 48; t++) {
                if (g.phase != TK_PHASE_PLAY) continue;
                u32 pos = g.trick_no * 4 + g.nt;
                if (pos != (u32)t) { fprintf(stderr, "slot %ld game %d card %d: position %u\n", i, e, t, pos); return 5; }
                if (rctr != rng_ctr(128u + pos).v) { fprintf(stderr, "slot %ld game %d card %d: carried counter differs from the rebuilt one\n", i, e, t); return 6; }
                u64 m = legal_now(g);
                u32 a = policy_action(key, RngCtr{rctr}, m);
                if (a != policy_action(key, pos, m)) { fprintf(stderr, "slot %ld game %d card %d: card from the carried counter\n", i, e, t); return 7; }
                if (g.nt && (TK_LO(m) == 0 || TK_HI(m) == 0)) {
                    u32 hs = TK_HI(m) ? ~0u : 0u;
                    if (policy_action_follow(key, RngCtr{rctr}, TK_LO(m) | TK_HI(m), hs) != a) return 8;
                }
                rctr += TK_RNG_STEP;
                actions[t] = (uint8_t)a;
                u64 sc = 0; u32 ti = 0;
                u32 nt = g.nt;
                int res = apply_step<true, true>(g, a, sc, ti, true);
                if (res < 0) { fprintf(stderr, "slot %ld game %d card %d: apply_step %d\n", i, e, t, res); return 9; }
                bool fin = res == 1;
                played++;
                if (fin) {                       // the renewal region: the next game's leader is not known here; the loop
                    rctr = rng_ctr(128u).v;      // rebuilds the observation word from the game it has unpacked (next pass)
                    // the finished game's own last observation is not written by the loop (the fresh game's is)
                    break;
                }
                if (nt < 3) ocar += TK_OBS_CARD;
                else ocar = obs_carry(g.leader, g.trick_no << 2);
                u64 legal = legal_now(g);
                u64 want = obs_word_with<true>(g, false, legal);
                u64 got = obs_word_with(ocar, g.error, 0u, legal);
                if (got != want) { fprintf(stderr, "slot %ld game %d card %d: observation word %016llx, want %016llx\n", i, e, t, (unsigned long long)got, (unsigned long long)want); return 10; }
                half[t] = (uint8_t)((obs_carry_hi(ocar) >> 22) & 0xFFu);
            }
            // the fresh game's word, as the 4th card's copy builds it after the renewal (checked at the top of the next pass)
            {
                u64 nkey = game_key(seed, offset + (u64)i, (u64)e + 1);
                u64 n0, n1, n2, n3, nt_;
                deal_thread(nkey, n0, n1, n2, n3, nt_);
                u32 nc, nd, nk;
                sample_setup(nkey, mix, nc, nd, nk);
                Game q;
                setup_game(q, n0, n1, n2, n3, nt_, nc, nd, nk);
                q.epar = 0; q.cprev = 0;
                if (q.phase == TK_PHASE_EXCHANGE) bot_exchange(q, nkey);
                ocar = obs_carry(q.leader, q.trick_no << 2);
                u64 legal = legal_now(q);
                if (obs_word_with(ocar, q.error, 1u, legal) != (obs_word_with<true>(q, false, legal) | (1ULL << 62))) return 11;
            }
            fwrite(actions, 1, 48, f); fwrite(half, 1, 48, f); fwrite(&played, 2, 1, f);
        }
    }
    fclose(f);
    return 0;
}
