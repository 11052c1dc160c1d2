// The follower-card forms of the trick-aligned card loops (tarok_amd/csrc/tarok_device.h: legal_mask_follow,
// kth_bit_word, hand_of<true> on a C plane that carries TK_C_PAD) run on the CPU, g++ with the gfx950 builtins
// emulated, for tests/test_follower_pick_host.py.
//   follower_pick_host pick                               kth_bit_word against kth_bit, exhaustive / sampled
//   follower_pick_host seed offset n episode mix out.bin  games played the way the trick-aligned loop plays them
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>

static int check_word(u32 w, bool high, unsigned long long &cases) {
    u64 m = high ? (u64)w << 32 : (u64)w;
    u32 n = (u32)__popc(w);
    for (u32 k = 0; k < n; k++, cases++) {
        u32 a = kth_bit_word(w, high ? ~0u : 0u, k), b = kth_bit(m, k);
        if (a != b || !((m >> a) & 1)) { fprintf(stderr, "kth_bit_word(%08x, %s, %u) = %u, kth_bit = %u\n", w, high ? "high" : "low", k, a, b); return 1; }
    }
    return 0;
}

// (a) every 8-bit pattern in each of the four suit bytes; seeded samples of non-zero subsets of up to 12 of the 22
// tarok bits (a hand holds 12 cards) and of up to 12 bits of the low word (the whole hand of a seat without
// taroks); every k below the popcount
static int pick_check() {
    unsigned long long cases = 0, masks = 0;
    for (int b = 0; b < 4; b++)
        for (u32 p = 1; p < 256; p++, masks++)
            if (check_word(p << (8 * b), false, cases)) return 1;
    u64 r = 0x2545F4914F6CDD1DULL;
    for (int it = 0; it < 240000; it++) {
        r ^= r << 13; r ^= r >> 7; r ^= r << 17;
        bool high = it % 6 != 5;                         // 200,000 tarok masks, 40,000 low-word hands
        u32 span = high ? 22u : 32u, n = 1 + (u32)((r >> 40) % 12), w = 0;
        u64 q = r * 0xD1B54A32D192ED03ULL;
        for (u32 j = 0; j < n; j++) { q ^= q << 13; q ^= q >> 7; q ^= q << 17; w |= 1u << (u32)((q >> 33) % span); }
        if (it % 5000 == 0 && high) w = 0x3FFFFFu & ~(~0u << (1 + (u32)(it / 5000) % 12));   // runs of low bits, the pagat among them
        if (it % 5000 == 1 && high) w = 1u << (it % 22);
        if (__popc(w) > 12 || w == 0) return 2;
        masks++;
        if (check_word(w, high, cases)) return 1;
    }
    printf("%llu masks, %llu picks\n", masks, cases);
    return 0;
}

static bool same_state(const Game &a, const Game &b) {
    return a.A == b.A && a.B == b.B && a.C == b.C && a.talon == b.talon && a.trick == b.trick && a.nt == b.nt && a.leader == b.leader &&
           a.trick_no == b.trick_no && a.phase == b.phase && a.contract == b.contract && a.tl == b.tl && a.error == b.error;
}

int main(int argc, char **argv) {
    if (argc == 2 && argv[1][0] == 'p') return pick_check();
    if (argc < 7) { fprintf(stderr, "usage: %s pick | seed offset n episode mix out.bin\n", argv[0]); return 2; }
    u64 seed = strtoull(argv[1], 0, 10), offset = strtoull(argv[2], 0, 10);
    long n = atol(argv[3]);
    u32 episode = (u32)atol(argv[4]);
    int mix = atoi(argv[5]);
    FILE *f = fopen(argv[6], "wb");
    if (!f) return 3;
    for (long i = 0; i < n; i++) {
        u64 key = game_key(seed, offset + (u64)i, episode);
        u64 h0, h1, h2, h3, tal;
        deal_thread(key, h0, h1, h2, h3, tal);
        u32 c, d, k;
        sample_setup(key, mix, c, d, k);
        Game g;                              // the generic path: legal_now, policy_action, apply_step
        setup_game(g, h0, h1, h2, h3, tal, c, d, k);
        g.epar = 0; g.cprev = 0;
        if (g.phase == TK_PHASE_EXCHANGE) bot_exchange(g, key);
        // the trick-aligned loop's path: the C plane padded for the length of the loop, the trick's cards from the
        // plane's gain, a follower's mask from legal_mask_follow and its card from the one-word pick
        Game p = g;
        p.C |= TK_C_PAD;
        u64 c_lead = 0, legal = legal_mask(hand_of<true>(p, p.leader), false, 0u, p.contract);
        u32 hi_sel = 0;
        u64 masks[48], fmasks[48];
        uint8_t hisel[48], actions[48];
        int16_t played = 0;
        for (int t = 0; t < 48; t++) {
            masks[t] = 0; fmasks[t] = 0; hisel[t] = 255; actions[t] = 255;
            if (g.phase != TK_PHASE_PLAY) continue;
            u32 nt = (u32)t & 3;
            if (p.phase != TK_PHASE_PLAY || p.nt != nt || g.nt != nt) { fprintf(stderr, "game %ld card %d: not trick-aligned\n", i, t); return 4; }
            u64 m = legal_now(g);
            masks[t] = m;
            u32 a;
            if (nt) {
                fmasks[t] = legal;
                hisel[t] = hi_sel == 0 ? 0 : (hi_sel == ~0u ? 1 : 2);
                a = policy_action_follow(key, (u32)t, TK_LO(legal) | TK_HI(legal), hi_sel);
            } else {
                if (legal != m) { fprintf(stderr, "game %ld card %d: the leader's mask from the padded plane differs\n", i, t); return 5; }
                a = policy_action(key, (u32)t, legal);
            }
            actions[t] = (uint8_t)a;
            if (a != policy_action(key, (u32)t, m)) { fprintf(stderr, "game %ld card %d: card %u, generic pick %u\n", i, t, a, policy_action(key, (u32)t, m)); return 6; }
            u64 s1 = 0, s2 = 0; u32 t1 = 0, t2 = 0;
            int r1 = apply_step<true, true>(g, a, s1, t1, true);
            if (nt == 0) c_lead = p.C;
            int r2 = apply_step<true, true>(p, a, s2, t2, true, &c_lead);
            Game q = p;
            q.C &= TK_DECK;
            if (r1 != r2 || t1 != t2 || !same_state(g, q) || (p.C & TK_C_PAD) != TK_C_PAD) { fprintf(stderr, "game %ld card %d: padded-plane state differs\n", i, t); return 7; }
            if (r1 == 1 && final_scores(g) != final_scores(q)) return 8;
            u32 seat = (p.leader + p.nt) & 3;
            if (hand_of<true>(p, seat) != hand_of(g, seat)) { fprintf(stderr, "game %ld card %d: hand from the padded plane differs\n", i, t); return 9; }
            if (p.phase == TK_PHASE_PLAY) {
                if (p.nt) legal = legal_mask_follow(hand_of<true>(p, seat), p.trick & 63, p.contract, hi_sel);
                else legal = legal_mask(hand_of<true>(p, p.leader), false, 0u, p.contract);
            }
            played++;
        }
        fwrite(masks, 8, 48, f); fwrite(fmasks, 8, 48, f); fwrite(hisel, 1, 48, f); fwrite(actions, 1, 48, f); fwrite(&played, 2, 1, f);
    }
    fclose(f);
    return 0;
}
