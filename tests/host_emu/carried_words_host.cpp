// The carried-word forms of the trick-aligned card loops (tarok_amd/csrc/tarok_device.h: FamilyWord, LeadWord, the error bit
// and the seat's smears in the observation carry, apply_step<.., .., CARRIED>) run on the CPU, g++ with the gfx950 builtins
// emulated, for tests/test_carried_words_host.py.
//   carried_words_host helpers                                    every new overload against the helper it replaces
//   carried_words_host seed offset n episode mix games out.bin   `games` games in a row per slot, played the way the
//                                                                 trick-aligned loop plays and renews them
#include "hip/hip_runtime.h"
#include "../../tarok_amd/csrc/tarok_device.h"
#include <stdio.h>
#include <stdlib.h>

struct Rng {
    u64 r;
    u32 next() { r ^= r << 13; r ^= r >> 7; r ^= r << 17; return (u32)((r * 0xD1B54A32D192ED03ULL) >> 32); }
    u32 below(u32 n) { return next() % n; }
};

static bool same_state(const Game &a, const Game &b) {
    return a.A == b.A && a.B == b.B && a.C == b.C && a.talon == b.talon && a.trick == b.trick && a.nt == b.nt && a.leader == b.leader &&
           a.trick_no == b.trick_no && a.phase == b.phase && a.contract == b.contract && a.tl == b.tl && a.error == b.error &&
           a.declarer == b.declarer && a.king == b.king && a.team == b.team;
}

#define FAIL(code, ...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return code; } while (0)

// One trick walked three ways from the same state: the per-card helpers as the loop used them before (O), the carried words
// (N) and, on a clean plane, the generic forms (legal_now, the trick's cards from the ids: I).  PAD: the C plane carries TK_C_PAD.
template <bool PAD>
static int walk_trick(const Game &g0, const u32 cards[4], unsigned long long &cases) {
    Game o = g0, n = g0, i = g0;
    if (PAD) { o.C |= TK_C_PAD; n.C |= TK_C_PAD; }
    const FamilyWord fam = family_word(n.contract);
    LeadWord led = LeadWord{0u};
    u32 car_o = obs_carry(o.leader, o.trick_no << 2), car_n = obs_carry(n.leader, n.trick_no << 2, n.error);
    if ((n.error != 0) != (car_n != car_o) || (n.error && !(car_n & 0x80u))) FAIL(20, "the carried error bit is not bit 7 of the carry");
    // the leader's mask and hand, before the first card
    {
        u64 ho = hand_of<PAD>(o, o.leader), hn = hand_of<PAD>(n, obs_carry_ma(car_n), obs_carry_mb(car_n));
        if (ho != hn) FAIL(21, "leader's hand differs");
        if (legal_mask(ho, false, 0u, o.contract) != legal_mask(hn, fam)) FAIL(22, "leader's mask differs, contract %u", n.contract);
        if (!PAD && legal_mask(hn, fam) != legal_now(i)) FAIL(23, "leader's mask differs from legal_now");
    }
    u64 cl_o = 0, cl_n = 0;
    for (u32 k = 0; k < 4; k++, cases++) {
        u32 a = cards[k];
        if (k == 0) { cl_o = o.C; cl_n = n.C; led = lead_word(a); }
        u64 so = 0, sn = 0, si = 0; u32 to = 0, tn = 0, ti = 0;
        int ro = apply_step<true, true>(o, a, so, to, true, &cl_o);
        int rn = apply_step<true, true, true>(n, a, sn, tn, true, &cl_n, fam, led);
        if (ro != rn || to != tn || !same_state(o, n)) FAIL(24, "apply_step differs: contract %u card %u of the trick, result %d / %d, trick_info %04x / %04x", n.contract, k, ro, rn, to, tn);
        if (k < 3 && (rn != 0 || tn != 0)) FAIL(25, "a card before the 4th ended something");
        if (!PAD) {
            int ri = apply_step<true, true>(i, a, si, ti, true);
            if (ri != rn || ti != tn || !same_state(i, n)) FAIL(26, "apply_step differs from the generic form: contract %u card %u", n.contract, k);
        }
        const u32 fin01 = (u32)rn;                                    // = over01
        if (k == 3 && fin01 != (u32)(n.phase == TK_PHASE_DONE)) FAIL(27, "over01 and the phase disagree");
        // the next seat's hand, mask and the observation word, as the loop forms them after the card
        if (k < 3) { car_o += TK_OBS_CARD; car_n += TK_OBS_CARD; }
        else { car_o = obs_carry(o.leader, o.trick_no << 2); car_n = obs_carry(n.leader, n.trick_no << 2, n.error); }
        u32 seat = (o.leader + o.nt) & 3;
        if (obs_carry_ma(car_n) != (u32)((int)(seat << 31) >> 31) || obs_carry_mb(car_n) != (u32)((int)(seat << 30) >> 31)) FAIL(28, "seat smears differ at card %u", k);
        u64 ho = hand_of<PAD>(o, seat), hn = hand_of<PAD>(n, obs_carry_ma(car_n), obs_carry_mb(car_n));
        if (ho != hn) FAIL(29, "hand differs at card %u", k);
        u64 lo_, ln_;
        u32 hs_o = 0x55u, hs_n = 0xAAu;
        if (k < 3) {
            lo_ = legal_mask_follow(ho, o.trick & 63, o.contract, hs_o);
            ln_ = legal_mask_follow(hn, led, fam, hs_n);
            if (hs_o != hs_n) FAIL(30, "hi_sel differs: contract %u lead %u", n.contract, cards[0]);
            if (ln_ != legal_mask(hn, true, cards[0], n.contract)) FAIL(31, "follower's mask differs from legal_mask");
        } else {
            lo_ = legal_mask(ho, false, 0u, o.contract);
            ln_ = legal_mask(hn, fam);
        }
        if (lo_ != ln_) FAIL(32, "legal mask differs: contract %u lead %u card %u: %016llx / %016llx", n.contract, cards[0], k, (unsigned long long)lo_, (unsigned long long)ln_);
        if (!PAD && n.phase == TK_PHASE_PLAY && ln_ != legal_now(i)) FAIL(33, "legal mask differs from legal_now");
        u64 wo = obs_word_with(car_o, o.error, fin01, lo_), wn = obs_word_with(car_n, fin01, ln_);
        if (wo != wn) FAIL(34, "observation word differs: %016llx / %016llx", (unsigned long long)wo, (unsigned long long)wn);
        if (!PAD && wn != (obs_word_with<true>(i, false, ln_) | ((u64)fin01 << 62))) FAIL(35, "observation word differs from the generic form");
        if ((u32)(wn >> 63) != n.error) FAIL(36, "error bit lost");
    }
    return 0;
}

// all ten contracts x every card led, random tricks on random states: hands of 0..12 cards (the seat that plays the trick's
// k-th card holds at least that card), both error values, all four leaders, padded and clean C planes
static int helpers_check() {
    Rng R{0x9E3779B97F4A7C15ULL};
    unsigned long long cases = 0, tricks = 0, ended = 0, gifts = 0;
    for (u32 contract = 0; contract < 10; contract++) {
        FamilyWord fam = family_word(contract);
        if ((fam.w & 1u) != ((0x281u >> contract) & 1u) || ((fam.w >> 22) & 1u) != ((0x280u >> contract) & 1u) ||
            (fam.w >> 31) != (contract == TK_KLOP ? 1u : 0u) || (fam.w & ~TK_FAM_MASK)) FAIL(10, "family word of contract %u: %08x", contract, fam.w);
        for (u32 lead = 0; lead < 54; lead++) {
            LeadWord lw = lead_word(lead);
            if (lw.m != (lead >= 32 ? 0u : 0xFFu << (lead & 24))) FAIL(11, "lead word of card %u: %08x", lead, lw.m);
            for (u32 rep = 0; rep < 48; rep++) {
                u32 perm[54];
                for (u32 j = 0; j < 54; j++) perm[j] = j;
                for (u32 j = 53; j > 0; j--) { u32 k = R.below(j + 1), t = perm[j]; perm[j] = perm[k]; perm[k] = t; }
                for (u32 j = 0; j < 54; j++) if (perm[j] == lead) { perm[j] = perm[0]; perm[0] = lead; }
                Game g = {};
                g.contract = contract; g.declarer = R.below(4); g.king = R.below(4); g.team = R.below(16);
                g.leader = rep & 3; g.error = (rep >> 2) & 1;
                g.trick_no = (rep % 6 == 5) ? 11 : R.below(12);
                g.tl = contract == TK_KLOP ? R.below(7) : R.below(8);
                g.phase = TK_PHASE_PLAY;
                u32 held[4] = {0, 0, 0, 0}, cards[4];
                const u32 played_of_4 = 1 + (rep >> 3) % 4;             // of the other cards, 1/4 .. 4/4 lie in a pile already
                for (u32 j = 0; j < 54; j++) {
                    u32 c = perm[j], owner, inpile;
                    if (j < 4) { owner = (g.leader + j) & 3; inpile = 0; cards[j] = c; }                 // the trick's four cards
                    else if (j < 10) { owner = R.below(4); inpile = 1; g.talon |= (u64)c << (6 * (j - 4)); }
                    else { owner = R.below(4); inpile = (R.below(4) < played_of_4 || held[owner] >= 12) ? 1u : 0u; }
                    if (!inpile) held[owner]++;
                    g.A |= (u64)(owner & 1) << c; g.B |= (u64)(owner >> 1) << c; g.C |= (u64)inpile << c;
                }
                Game before = g;
                int rc = walk_trick<false>(g, cards, cases);
                if (!rc) rc = walk_trick<true>(g, cards, cases);
                if (rc) return rc;
                tricks++;
                // (what the sample reaches: games that end with this trick, and talon gifts)
                u64 s = 0; u32 t = 0;
                int r = 0;
                for (u32 k = 0; k < 4; k++) r = apply_step<true, true>(before, cards[k], s, t, true);
                ended += (u32)r;
                gifts += (contract == TK_KLOP && g.tl != before.tl) ? 1u : 0u;
            }
        }
    }
    if (!ended || !gifts || ended == tricks) FAIL(12, "the sample misses a case: %llu tricks, %llu ended, %llu gifts", tricks, ended, gifts);
    printf("%llu tricks, %llu cards, %llu games ended, %llu gifts\n", tricks, cases, ended, gifts);
    return 0;
}

static void fresh_game(Game &g, u64 &key, u64 seed, u64 gidx, u32 episode, int mix, u32 error) {
    key = game_key(seed, gidx, episode);
    u64 h0, h1, h2, h3, tal;
    deal_thread(key, h0, h1, h2, h3, tal);
    u32 c, d, k;
    sample_setup(key, mix, c, d, k);
    setup_game(g, h0, h1, h2, h3, tal, c, d, k);
    g.epar = 0; g.cprev = 0;
    if (g.phase == TK_PHASE_EXCHANGE) bot_exchange(g, key);
    g.error = error;
}

int main(int argc, char **argv) {
    if (argc == 2 && argv[1][0] == 'h') return helpers_check();
    if (argc < 8) { fprintf(stderr, "usage: %s helpers | seed offset n episode mix games out.bin\n", argv[0]); return 2; }
    u64 seed = strtoull(argv[1], 0, 10), offset = strtoull(argv[2], 0, 10);
    long n = atol(argv[3]);
    u32 episode = (u32)atol(argv[4]);
    int mix = atoi(argv[5]), games = atoi(argv[6]);
    FILE *f = fopen(argv[7], "wb");
    if (!f) return 3;
    for (long i = 0; i < n; i++) {
        // the error bit a game starts with: differs between a slot's successive games (a fresh line carries none in the
        // library; unpack_fresh reads the bit all the same, and a launch may start from a state that has it set)
        auto err_of = [&](int k) { return (u32)((i + k) % 3 == 0); };
        u64 key, rkey;
        Game g, r;                          // g: the loop's state (padded plane, carried words); r: the generic path
        fresh_game(r, rkey, seed, offset + (u64)i, episode, mix, err_of(0));
        g = r; key = rkey;
        // ---- tricks(): in front of the loop
        g.C |= TK_C_PAD;
        u32 rctr = rng_ctr(128u + g.trick_no * 4).v;
        u32 ocar = obs_carry(g.leader, g.trick_no << 2, g.error);
        FamilyWord fam = family_word(g.contract);
        LeadWord led = LeadWord{0u};
        u64 c_lead = 0, legal = legal_mask(hand_of<true>(g, g.leader), false, 0u, g.contract);
        u32 legal_hi = 0;
        int game = 0;
        u64 masks[48], obs[48];
        uint8_t actions[48];
        int16_t scores[4], played = 0;
        for (int t = 0; t < 48; t++) { masks[t] = 0; obs[t] = 0; actions[t] = 255; }
        while (game < games) {
            for (u32 nt = 0; nt < 4; nt++) {
                if (g.nt != nt || r.nt != nt || r.phase != TK_PHASE_PLAY || played >= 48) { fprintf(stderr, "slot %ld: not trick-aligned\n", i); return 4; }
                // the generic path's view of the card
                u64 m = legal_now(r);
                u32 pos = r.trick_no * 4 + r.nt;
                if (pos != (u32)played) return 5;
                if (legal != m) { fprintf(stderr, "slot %ld game %d card %d: carried mask %016llx, legal_now %016llx\n", i, game, played, (unsigned long long)legal, (unsigned long long)m); return 6; }
                u32 a = nt ? policy_action_follow(key, RngCtr{rctr}, TK_LO(legal) | TK_HI(legal), legal_hi) : policy_action(key, RngCtr{rctr}, legal);
                rctr += TK_RNG_STEP;
                if (a != policy_action(rkey, pos, m)) { fprintf(stderr, "slot %ld game %d card %d: card differs\n", i, game, played); return 7; }
                masks[played] = m; actions[played] = (uint8_t)a;
                if (nt == 0) { c_lead = g.C; led = lead_word(a); }
                u64 s1 = 0, s2 = 0; u32 t1 = 0, t2 = 0;
                int res = apply_step<true, true, true>(g, a, s1, t1, true, &c_lead, fam, led);
                int rr = apply_step<true, true>(r, a, s2, t2, true);
                Game q = g; q.C &= TK_DECK;
                if (res != rr || t1 != t2 || !same_state(q, r) || (g.C & TK_C_PAD) != TK_C_PAD) { fprintf(stderr, "slot %ld game %d card %d: state differs\n", i, game, played); return 8; }
                const int at = played++;
                if (nt == 3 && res == 1) {
                    // ---- the renewal region: queue entry (scored here), swap_in of a freshly set-up game through its line
                    u64 sc = final_scores(q);
                    if (sc != final_scores(r)) return 9;
                    for (int s = 0; s < 4; s++) scores[s] = (int16_t)(sc >> (16 * s));
                    game++;
                    Game nx; u64 nkey;
                    fresh_game(nx, nkey, seed, offset + (u64)i, episode + (u32)game, mix, err_of(game));
                    u64 x0, x1, y0, y1;
                    pack(nx, x0, x1, y0, y1);
                    unpack_fresh(g, x0, x1, y0, y1);
                    g.C |= TK_C_PAD;
                    key = nkey;
                    rctr = rng_ctr(128u).v;
                    fam = family_word(g.contract);
                    r = nx; rkey = nkey;
                    q = g; q.C &= TK_DECK;
                    if (!same_state(q, r)) return 10;
                }
                // ---- the next card's mask and the observation, from the carried words
                if (nt < 3) ocar += TK_OBS_CARD;
                else ocar = obs_carry(g.leader, g.trick_no << 2, g.error);
                u64 hand = hand_of<true>(g, obs_carry_ma(ocar), obs_carry_mb(ocar));
                if (hand != hand_of(r, (r.leader + r.nt) & 3)) return 11;
                if (nt < 3) legal = legal_mask_follow(hand, led, fam, legal_hi);
                else legal = legal_mask(hand, fam);
                u64 w = obs_word_with(ocar, (u32)res, legal);
                if (w != (obs_word_with<true>(r, false, legal_now(r)) | ((u64)(u32)res << 62))) { fprintf(stderr, "slot %ld game %d card %d: observation word differs\n", i, game, at); return 12; }
                obs[at] = w;
                if (nt == 3 && res == 1) {
                    fwrite(masks, 8, 48, f); fwrite(obs, 8, 48, f); fwrite(actions, 1, 48, f); fwrite(scores, 2, 4, f); fwrite(&played, 2, 1, f);
                    for (int t = 0; t < 48; t++) { masks[t] = 0; obs[t] = 0; actions[t] = 255; }
                    played = 0;
                }
            }
        }
    }
    fclose(f);
    return 0;
}
