// Device-side Tarok rules on bit-packed per-game lanes (gfx950 / CDNA4 only).
//
// One game = 4 x uint64, kept as two 16-byte pairs in two SoA arrays so a wave
// reads/writes 1 KiB contiguous per instruction:
//
//   play pair (rewritten by every card)
//     X0 = C plane [53:0] | n_in_trick<<54 (2) | leader<<56 (2) | trick_no<<58 (4) | phase<<62 (2)
//     X1 = talon 6x6-bit ids [35:0] | current trick 4x6-bit ids [59:36] | tl<<60 (3) | error<<63
//   seat pair (rewritten only when a trick is resolved: every 4th card)
//     Y0 = A plane [53:0] | contract<<54 (4) | declarer<<58 (2) | king<<60 (2) | cprev[3:2]<<62
//     Y1 = B plane [53:0] | team<<54 (4) | epar<<58 (4) | cprev[1:0]<<62
//          epar = the slot's episode number mod TK_AHEAD: says which of the slot's next-game
//          lines holds the next game; cprev = how many of them (the farthest ahead) were put
//          on a refill list by the previous launch, i.e. are being re-dealt during this one
//
// Card c (bit c of every plane) belongs to seat (B_c A_c).  C_c = 0: it is in
// that seat's hand (Igralec.roka).  C_c = 1: it has left the hands — it lies in
// that seat's won pile (Igralec.kupcek), or on the table (attributed to whoever
// played it until the trick is resolved), or it is a talon card nobody owns yet
// (parked in an opponent's pile bits; told apart through the ordered talon ids).
// `tl` is Klop's len(self.talon) (Klop.py:67) or, for Tri..Solo_ena, the chosen
// talon group (7 = none yet).
//
// Reference rules cited per function; the CPU statement of the same rules is
// oracle/tarok_oracle.c (test infrastructure, never linked here).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned long long u64;
typedef uint32_t u32;

// gfx950 ERRATUM GUARD (DESIGN.md §3 "the refill-role bug", tarok_amd/isa_check.py, profiles/r04_refill_root_cause.txt).
// v_lshlrev_b64 / v_lshrrev_b64 / v_ashrrev_i64 shift by v0 instead of by their amount register when that register is the
// LAST VGPR the wave was allocated (gfx90a's "Shift64HighRegBug"; ROCm 7.2.0's compiler works round it on gfx90a only).
// Every kernel of this library is declared TK_KERNEL(threads, B) — it may use v0 .. v(B-2) only — and starts with
// TK_VGPR_TOP(B, B-1), which marks v(B-1) used: the wave's allocation is always exactly B registers (B a multiple of the
// allocation granule, 8) and no value ever lives in the last one.  B is the kernel's occupancy bucket (<= 64: 8 waves per
// SIMD, 80: 6, 96: 5, 128: 4, 168: 3, 256: 2), so the guard costs one register of the bucket and no occupancy.  (A kernel
// that needs more than 256 registers — k_learn_dw — holds the rest in accumulation registers, which follow the VGPRs in the
// unified file: the row behind its last VGPR is always allocated.)
#define TK_VGPR_BUDGET(B) __attribute__((amdgpu_num_vgpr((B) - 1)))
#define TK_KERNEL(threads, B) __global__ __launch_bounds__(threads) TK_VGPR_BUDGET(B)
#define TK_VGPR_STR2(x) #x
#define TK_VGPR_STR(x) TK_VGPR_STR2(x)
#define TK_VGPR_TOP(B, TOP)                                                                                           \
    do {                                                                                                              \
        static_assert((B) % 8 == 0 && (B) <= 256 && (TOP) == (B) - 1, "TK_VGPR_TOP(B, B - 1), B a multiple of 8");     \
        asm volatile("" ::: "v" TK_VGPR_STR(TOP));                                                                    \
    } while (0)

#define TK_BIT(i) (1ULL << (i))
#define TK_DECK ((1ULL << 54) - 1)
#define TK_TAROK (((1ULL << 22) - 1) << 32)
#define TK_PAGAT TK_BIT(32)
// Roka.vrednost_stiha card values (Roka.py:76-95)
#define TK_V5 (TK_BIT(7) | TK_BIT(15) | TK_BIT(23) | TK_BIT(31) | TK_BIT(32) | TK_BIT(52) | TK_BIT(53))
#define TK_V4 (TK_BIT(6) | TK_BIT(14) | TK_BIT(22) | TK_BIT(30))
#define TK_V3 (TK_BIT(5) | TK_BIT(13) | TK_BIT(21) | TK_BIT(29))
#define TK_V2 (TK_BIT(4) | TK_BIT(12) | TK_BIT(20) | TK_BIT(28))
// Roka.mozno_zalozit (Roka.py:23-27) with Karta.vrednost (Karta.py:10-16):
// suit ranks 1..7 and taroks 2..7
#define TK_DISCARDABLE (0x7F7F7F7FULL | (0x3FULL << 33))

enum { TK_KLOP = 0, TK_TRI, TK_DVE, TK_ENA, TK_SOLO_TRI, TK_SOLO_DVE, TK_SOLO_ENA, TK_BERAC, TK_SOLO_BREZ, TK_ODPRTI_BERAC };
enum { TK_PHASE_EXCHANGE = 1, TK_PHASE_PLAY = 2, TK_PHASE_DONE = 3 };

struct Game {
    u64 A, B, C, talon;
    u32 trick, nt, leader, trick_no, phase, contract, declarer, king, error, team, tl, epar, cprev;
};

// (x0, x1) = play pair, (y0, y1) = seat pair
__device__ __forceinline__ void unpack(Game &g, u64 x0, u64 x1, u64 y0, u64 y1) {
    g.C = x0 & TK_DECK; g.A = y0 & TK_DECK; g.B = y1 & TK_DECK;
    u32 m0 = (u32)(x0 >> 54), m2 = (u32)(y0 >> 54), m3 = (u32)(y1 >> 54);
    g.nt = m0 & 3; g.leader = (m0 >> 2) & 3; g.trick_no = (m0 >> 4) & 15; g.phase = m0 >> 8;
    g.talon = x1 & ((1ULL << 36) - 1);
    g.trick = (u32)(x1 >> 36) & 0xFFFFFF;
    g.tl = (u32)(x1 >> 60) & 7; g.error = (u32)(x1 >> 63);
    g.contract = m2 & 15; g.declarer = (m2 >> 4) & 3; g.king = (m2 >> 6) & 3;
    g.team = m3 & 15; g.epar = (m3 >> 4) & 15; g.cprev = (m3 >> 8) | ((m2 >> 8) << 2);
}

// The same for a line of the dealt-ahead buffer: a game at its first card (deal_into_buffer: setup_game, Bot
// exchange), so no card of a trick and nothing to re-deal.  Written as constants: where the caller is at the end
// of a trick of EVERY lane (the trick-aligned card loops) "no card led" stays a compile-time fact across the
// swap, and the next legal mask is the leader's (the hand, pagat rule) without the follow-suit selects.
__device__ __forceinline__ void unpack_fresh(Game &g, u64 x0, u64 x1, u64 y0, u64 y1) {
    g.C = x0 & TK_DECK; g.A = y0 & TK_DECK; g.B = y1 & TK_DECK;
    u32 m0 = (u32)(x0 >> 54), m2 = (u32)(y0 >> 54), m3 = (u32)(y1 >> 54);
    g.nt = 0; g.leader = (m0 >> 2) & 3; g.trick_no = (m0 >> 4) & 15; g.phase = m0 >> 8;
    g.talon = x1 & ((1ULL << 36) - 1);
    g.trick = 0;
    g.tl = (u32)(x1 >> 60) & 7; g.error = (u32)(x1 >> 63);
    g.contract = m2 & 15; g.declarer = (m2 >> 4) & 3; g.king = (m2 >> 6) & 3;
    g.team = m3 & 15; g.epar = (m3 >> 4) & 15; g.cprev = 0;
}

// (g.C must be a clean plane here, bits 54-63 zero: the trick-aligned card loops keep TK_C_PAD set in their working
// copy — hand_of<true> — and take it off before the plane reaches pack_play / store_game or, through the finished-games
// ring, score_game.  A padded plane would be or-ed over nt, leader, trick_no and phase.)
__device__ __forceinline__ void pack_play(const Game &g, u64 &x0, u64 &x1) {
    x0 = g.C | ((u64)(g.nt | (g.leader << 2) | (g.trick_no << 4) | (g.phase << 8)) << 54);
    x1 = g.talon | ((u64)g.trick << 36) | ((u64)g.tl << 60) | ((u64)g.error << 63);
}
__device__ __forceinline__ void pack_seats(const Game &g, u64 &y0, u64 &y1) {
    y0 = g.A | ((u64)(g.contract | (g.declarer << 4) | (g.king << 6) | ((g.cprev >> 2) << 8)) << 54);
    y1 = g.B | ((u64)(g.team | (g.epar << 4) | ((g.cprev & 3) << 8)) << 54);
}
__device__ __forceinline__ void pack(const Game &g, u64 &x0, u64 &x1, u64 &y0, u64 &y1) {
    pack_play(g, x0, x1);
    pack_seats(g, y0, y1);
}

__device__ __forceinline__ int popc64(u64 m) { return __popcll(m); }

// v_bitop3_b32: any boolean function of three 32-bit words in one instruction.  The immediate
// is the function's truth table, written here by evaluating it on the three selector bytes.
template <class F> constexpr u32 tk_tt(F f) { return f(0xF0u, 0xCCu, 0xAAu) & 0xFFu; }
#define TK_BITOP3(a, b, c, ...) ((u32)__builtin_amdgcn_bitop3_b32((a), (b), (c), tk_tt([](u32 a_, u32 b_, u32 c_) { return (__VA_ARGS__); })))
#define TK_LO(x) ((u32)(x))
#define TK_HI(x) ((u32)((x) >> 32))
#ifndef TK_KEEP_VGPR                         // value materialised in a VGPR here (the CPU build of the tests defines it away)
#define TK_KEEP_VGPR(x) asm volatile("" : "+v"(x))
#endif
#define TK_U64(lo, hi) (((u64)(u32)(hi) << 32) | (u64)(u32)(lo))

__device__ __forceinline__ u64 seat_cards(const Game &g, u32 s) {
    u64 a = (s & 1) ? g.A : ~g.A, b = (s & 2) ? g.B : ~g.B;
    return a & b & TK_DECK;
}
// hand of seat s = ~C & (A == s&1) & (B == s>>1): with ma / mb = all-ones when the seat bit is
// set, (A xnor ma) & (B xnor mb) & ~C is two v_bitop3 per 32-bit half
// C_PADDED: the caller keeps the ten bits above the deck of the C plane's high word set (TK_C_PAD; the trick-aligned
// card loops do, from their first card to their last): ~C then clears them in every hand, without the mask
#define TK_C_PAD (0xFFC00000ULL << 32)
template <bool C_PADDED = false>
__device__ __forceinline__ u64 hand_of(const Game &g, u32 s) {
    u32 ma = (u32)((int)(s << 31) >> 31), mb = (u32)((int)(s << 30) >> 31);
    u32 tl = TK_BITOP3(TK_LO(g.A), ma, TK_LO(g.C), ~c_ & ~(a_ ^ b_));
    u32 th = TK_BITOP3(TK_HI(g.A), ma, TK_HI(g.C), ~c_ & ~(a_ ^ b_));
    u32 hl = TK_BITOP3(tl, TK_LO(g.B), mb, a_ & ~(b_ ^ c_));
    u32 hh = TK_BITOP3(th, TK_HI(g.B), mb, a_ & ~(b_ ^ c_));
    if (!C_PADDED) hh &= 0x3FFFFFu;
    return TK_U64(hl, hh);
}
// the same from the seat's two smears, for a caller that carries them from card to card
template <bool C_PADDED = false>
__device__ __forceinline__ u64 hand_of(const Game &g, u32 ma, u32 mb) {
    u32 tl = TK_BITOP3(TK_LO(g.A), ma, TK_LO(g.C), ~c_ & ~(a_ ^ b_));
    u32 th = TK_BITOP3(TK_HI(g.A), ma, TK_HI(g.C), ~c_ & ~(a_ ^ b_));
    u32 hl = TK_BITOP3(tl, TK_LO(g.B), mb, a_ & ~(b_ ^ c_));
    u32 hh = TK_BITOP3(th, TK_HI(g.B), mb, a_ & ~(b_ ^ c_));
    if (!C_PADDED) hh &= 0x3FFFFFu;
    return TK_U64(hl, hh);
}
// won pile of seat S (incl. whatever is parked in its pile bits): C & (A == S&1) & (B == S>>1)
template <int S> __device__ __forceinline__ u64 pile_of(const Game &g) {
    u32 l, h;
    if (S == 0)      { l = TK_BITOP3(TK_LO(g.A), TK_LO(g.B), TK_LO(g.C), ~a_ & ~b_ & c_); h = TK_BITOP3(TK_HI(g.A), TK_HI(g.B), TK_HI(g.C), ~a_ & ~b_ & c_); }
    else if (S == 1) { l = TK_BITOP3(TK_LO(g.A), TK_LO(g.B), TK_LO(g.C), a_ & ~b_ & c_);  h = TK_BITOP3(TK_HI(g.A), TK_HI(g.B), TK_HI(g.C), a_ & ~b_ & c_); }
    else if (S == 2) { l = TK_BITOP3(TK_LO(g.A), TK_LO(g.B), TK_LO(g.C), ~a_ & b_ & c_);  h = TK_BITOP3(TK_HI(g.A), TK_HI(g.B), TK_HI(g.C), ~a_ & b_ & c_); }
    else             { l = TK_BITOP3(TK_LO(g.A), TK_LO(g.B), TK_LO(g.C), a_ & b_ & c_);   h = TK_BITOP3(TK_HI(g.A), TK_HI(g.B), TK_HI(g.C), a_ & b_ & c_); }
    return TK_U64(l, h);
}

__device__ __forceinline__ u64 ids_mask(u64 ids, int first, int n) {
    u64 m = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
        if (i >= first && i < first + n) m |= 1ULL << ((ids >> (6 * i)) & 63);
    return m;
}
__device__ __forceinline__ u64 talon_all(const Game &g) { return ids_mask(g.talon, 0, 6); }

__device__ __forceinline__ bool klop_family(u32 c) { return c == TK_KLOP || c == TK_BERAC || c == TK_ODPRTI_BERAC; }
__device__ __forceinline__ bool has_exchange(u32 c) { return c >= TK_TRI && c <= TK_SOLO_ENA; }
__device__ __forceinline__ bool has_king(u32 c) { return c >= TK_TRI && c <= TK_ENA; }
// odpri_talon's korak (Navadna_igra.py:36-44) for Tri..Solo_ena: 3,2,1,3,2,1
__device__ __forceinline__ u32 group_size(u32 c) { return 3 - ((c - 1) % 3); }

// talon cards that sit in nobody's pile yet
__device__ __forceinline__ u64 talon_unowned(const Game &g) {
    if (g.contract == TK_KLOP) return ids_mask(g.talon, 0, (int)g.tl);
    if (has_exchange(g.contract) && g.tl != 7) {
        u32 gs = group_size(g.contract);
        return talon_all(g) & ~ids_mask(g.talon, (int)(g.tl * gs), (int)gs);
    }
    return talon_all(g);
}

// Roka.prestej (Roka.py:56-98), order independent:
// sum(val) - 2*floor(n/3) - [n%3 != 0].  The values 1..5 are summed as nested
// popcounts (v_bcnt accumulates for free); n <= 54 so n/3 = (n*43)>>7.
__device__ __forceinline__ int prestej(u64 m) {
    // suits = low word (rank r of a suit is bit r-1 of its byte: ranks 5..8 are worth 2..5),
    // taroks = high word (pagat, mond, skis = bits 0, 20, 21 are worth 5, the others 1)
    u32 lo = TK_LO(m), hi = TK_HI(m);
    u32 n = (u32)__popc(lo) + (u32)__popc(hi);
    u32 v = n + (u32)__popc(lo & 0xF0F0F0F0u) + (u32)__popc(lo & 0xE0E0E0E0u) + (u32)__popc(lo & 0xC0C0C0C0u) +
            (u32)__popc(lo & 0x80808080u) + 4u * (u32)__popc(hi & 0x300001u);
    u32 q = (n * 43u) >> 7;
    return (int)(v - 2 * q - (n != 3 * q ? 1u : 0u));
}

// mozne_karte: Navadna_igra.py:158-168; Klop.py:96-133 adds "pagat only when
// nothing else is allowed" (the over-play filter there is dead code).
// The suits are the low word of a plane and the taroks (pagat = bit 0) the high word, so the
// rule is written on the halves: lead-suit cards if any, else taroks if any, else the hand.
// Written on word masks, not on compares and selects: on gfx950 a select costs a lone wave 16.6 cycles through a
// compare (v_cmp, two idle slots, v_cndmask), 28.5 on a compound condition (v_cmp, s_and, v_cndmask) and 12.5 as
// three plain vector instructions (tools/valu_issue: cmpsel / select / arithsel).
// all ones where x == 0, in two plain vector instructions: v_sad_u8 sums the four bytes of x onto -1, the sign
// of that is smeared over the word.  (Written as min(x, 1) or as a sign trick of x itself the compiler turns it
// back into the compare and the select; it does not look into v_sad_u8.)
__device__ __forceinline__ u32 tk_zero_mask(u32 x) { return (u32)((int)__builtin_amdgcn_sad_u8(x, 0u, ~0u) >> 31); }
__device__ __forceinline__ u64 legal_mask(u64 hand, bool has_lead, u32 lead, u32 contract) {
    u32 hl = TK_LO(hand), hh = TK_HI(hand);
    u32 lm = has_lead ? ~0u : 0u;                       // (a compile-time fact in the trick-aligned card loops)
    u32 tarok_led = (u32)((int)(lead << 26) >> 31);     // bit 5 of the id: no suit to follow, taroks next
    u32 s = TK_BITOP3(hl, 0xFFu << (lead & 24), tarok_led, a_ & b_ & ~c_) & lm;
    u32 zs = tk_zero_mask(s);                           // no card of the suit led (or nobody led)
    u32 zt = tk_zero_mask(hh) | ~lm;                    // no taroks (or nobody led)
    u32 bl = s | TK_BITOP3(hl, zs, zt, a_ & b_ & c_);
    u32 bh = hh & zs;
    u32 kf = (0x281u >> contract) & 1u;                 // Klop, Berac, Odprti berac: the pagat only when nothing else goes
    u32 only_pagat = tk_zero_mask(bl | (bh & ~1u));
    return TK_U64(bl, TK_BITOP3(bh, kf, only_pagat, a_ & ~(b_ & ~c_)));
}

// The same rule for a seat that FOLLOWS (somebody has led).  Then all legal cards lie in one word: cards of the suit
// led or, without taroks, the whole hand — the low word; taroks, when the seat has no card of the suit (the pagat rule
// only ever clears bit 0 of them) — the high word.  hi_sel: all ones when it is the high word, else zero.
__device__ __forceinline__ u64 legal_mask_follow(u64 hand, u32 lead, u32 contract, u32 &hi_sel) {
    u32 hl = TK_LO(hand), hh = TK_HI(hand);
    u32 tarok_led = (u32)((int)(lead << 26) >> 31);
    u32 s = TK_BITOP3(hl, 0xFFu << (lead & 24), tarok_led, a_ & b_ & ~c_);
    u32 zs = tk_zero_mask(s);                           // no card of the suit led
    u32 zt = tk_zero_mask(hh);                          // no taroks
    u32 bl = s | TK_BITOP3(hl, zs, zt, a_ & b_ & c_);
    u32 bh = hh & zs;
    u32 kf = (0x281u >> contract) & 1u;
    u32 only_pagat = tk_zero_mask(bl | (bh & ~1u));
    // zs & ~zt, as one opaque bit operation and pinned as a word: left to itself the compiler recognises the two sign
    // smears behind it and rebuilds this line, or the pick's last step hi_sel & 32, as a compare and a select — the
    // pair this rule code is written to avoid (see above)
    hi_sel = TK_BITOP3(zs, zt, zt, a_ & ~b_);           TK_KEEP_VGPR(hi_sel);
    return TK_U64(bl, TK_BITOP3(bh, kf, only_pagat, a_ & ~(b_ & ~c_)));
}

// CARRIED WORDS.  A caller that plays a game card by card (the trick-aligned card loops) rebuilds nothing that only
// changes with the game or with the trick: it keeps the words below and hands them to the overloads that follow.
//   FamilyWord, once per game: the three facts of the contract the rules ask for, in ONE word read off a constant by
//   the contract's number (two instructions where a game is taken): bit 0 = Klop, Berac or Odprti berac (the pagat
//   rule; the legal masks and it as it is, for the high word of a hand has nothing above bit 21 and so bits 22 and 31
//   clear nothing there), bit 22 = Berac or Odprti berac (the game ends with the declarer's first trick), bit 31 = Klop
//   (the talon's gifts).  The constant: bits 0, 7, 9 | bits 22 + 7, 22 + 9 | bit 31, and nothing else within ten
//   bits above any of the three places.
//   LeadWord, once per trick: the byte of the suit led within a hand's low word, or zero where a tarok was led.
#define TK_FAM_LUT 0xA0000281u
#define TK_FAM_MASK 0x80400001u
struct FamilyWord { u32 w; };
struct LeadWord { u32 m; };
__device__ __forceinline__ FamilyWord family_word(u32 contract) {
    u32 w = (TK_FAM_LUT >> contract) & TK_FAM_MASK;     TK_KEEP_VGPR(w);
    return FamilyWord{w};
}
__device__ __forceinline__ LeadWord lead_word(u32 lead) {
    // (the smear pinned as a word: left to itself the compiler tests bit 5 of the id with a compare and selects)
    u32 tarok_led = (u32)((int)(lead << 26) >> 31);     TK_KEEP_VGPR(tarok_led);
    return LeadWord{(0xFFu << (lead & 24)) & ~tarok_led};
}
// legal_mask for the seat that LEADS (nobody has led: the hand, less the pagat where the rule holds)
__device__ __forceinline__ u64 legal_mask(u64 hand, FamilyWord fam) {
    u32 hl = TK_LO(hand), hh = TK_HI(hand);
    u32 only_pagat = tk_zero_mask(hl | (hh & ~1u));
    return TK_U64(hl, TK_BITOP3(hh, fam.w, only_pagat, a_ & ~(b_ & ~c_)));
}
// legal_mask_follow from the trick's LeadWord
__device__ __forceinline__ u64 legal_mask_follow(u64 hand, LeadWord lead, FamilyWord fam, u32 &hi_sel) {
    u32 hl = TK_LO(hand), hh = TK_HI(hand);
    u32 s = hl & lead.m;
    u32 zs = tk_zero_mask(s);                           // no card of the suit led
    u32 zt = tk_zero_mask(hh);                          // no taroks
    u32 bl = s | TK_BITOP3(hl, zs, zt, a_ & b_ & c_);
    u32 bh = hh & zs;
    u32 only_pagat = tk_zero_mask(bl | (bh & ~1u));
    hi_sel = TK_BITOP3(zs, zt, zt, a_ & ~b_);           TK_KEEP_VGPR(hi_sel);      // (see legal_mask_follow above)
    return TK_U64(bl, TK_BITOP3(bh, fam.w, only_pagat, a_ & ~(b_ & ~c_)));
}

__device__ __forceinline__ u64 legal_now(const Game &g) {
    u32 seat = (g.leader + g.nt) & 3;
    return legal_mask(hand_of(g, seat), g.nt != 0, g.trick & 63, g.contract);
}

// observation word (tarok_env.h TAROK_OBS_*) from an already computed legal mask
// (IN_PLAY: the caller knows that the game is not in the DONE phase)
template <bool IN_PLAY = false>
__device__ __forceinline__ u64 obs_word_with(const Game &g, bool finished_now, u64 legal) {
    u64 o = legal;
    o |= (u64)((g.leader + g.nt) & 3) << 54;
    o |= (u64)(g.trick_no * 4 + g.nt) << 56;
    if (IN_PLAY) o |= (u64)(finished_now ? 1u : 0u) << 62;               // (a shift of the caller's 0 / 1, no select)
    else if (finished_now || g.phase == TK_PHASE_DONE) o |= 1ULL << 62;
    o |= (u64)g.error << 63;
    return o;
}

// The seat and position bits of the observation word (54..61) for a caller that plays a game card by card, as ONE
// carried word: the position (cards played, 0..47) in bits 0..5 and the seat to play in bits 30..31, so that one add
// of TK_OBS_CARD moves both — the seat's carry falls off the top of the word instead of into the position.  Turned
// right by eight bits it is the observation's high word: position at bit 24, seat at bit 22.  After a trick's 4th
// card the seat is the trick's winner, not the next one round: the word is rebuilt there (obs_carry).
#define TK_OBS_CARD ((1u << 30) + 1u)
__device__ __forceinline__ u32 obs_carry(u32 seat, u32 pos) { return (seat << 30) | pos; }
__device__ __forceinline__ u32 obs_carry_hi(u32 carry) { return (carry >> 8) | (carry << 24); }
// the observation word of a game in play from the carried word (fin01: the game ended with this card, 0 / 1)
__device__ __forceinline__ u64 obs_word_with(u32 carry, u32 error, u32 fin01, u64 legal) {
    return legal | ((u64)(obs_carry_hi(carry) | (fin01 << 30) | (error << 31)) << 32);
}

// The same with the game's error bit carried IN the word, already shifted: bit 7 of the carried word is bit 31 of the
// observation's high word after the turn (and bit 6, which the position never reaches — 47 cards at the most — is
// where the turn takes bit 30 from: it stays clear).  The error bit only changes where a game is taken: no shift and
// no or per card.  The seat's two smears (hand_of) are read off the same word.
__device__ __forceinline__ u32 obs_carry(u32 seat, u32 pos, u32 error) { return (error << 7) | obs_carry(seat, pos); }
__device__ __forceinline__ u32 obs_carry_ma(u32 carry) { return (u32)((int)(carry << 1) >> 31); }
__device__ __forceinline__ u32 obs_carry_mb(u32 carry) { return (u32)((int)carry >> 31); }
__device__ __forceinline__ u64 obs_word_with(u32 carry_with_error, u32 fin01, u64 legal) {
    return legal | ((u64)(obs_carry_hi(carry_with_error) | (fin01 << 30)) << 32);
}

// observation word (tarok_env.h TAROK_OBS_*)
__device__ __forceinline__ u64 obs_word(const Game &g, bool finished_now) {
    bool play = g.phase == TK_PHASE_PLAY;
    u64 o = play ? legal_now(g) : 0;
    o |= (u64)((g.leader + g.nt) & 3) << 54;
    o |= (u64)(g.trick_no * 4 + g.nt) << 56;
    if (finished_now || g.phase == TK_PHASE_DONE) o |= 1ULL << 62;
    o |= (u64)g.error << 63;
    return o;
}

__device__ __forceinline__ u64 pack_scores(int s0, int s1, int s2, int s3) {
    return (u64)(uint16_t)(int16_t)s0 | ((u64)(uint16_t)(int16_t)s1 << 16) |
           ((u64)(uint16_t)(int16_t)s2 << 32) | ((u64)(uint16_t)(int16_t)s3 << 48);
}

// End-of-game scoring, Klop and Navadna/Solo in one straight-line pass (lanes of a
// wave finish different contracts in the same step; two separate routines would
// both be paid by every such wave).
//   Klop (Klop.py:36-45): -points each; if anybody took more than 35 everybody
//     scores 0 (the -70 branch at Klop.py:39-40 is unreachable).
//   Navadna/Solo (Navadna_igra.py:80-113): team pile (+ the talon rest only in the
//     narrow case of :87), v -> sign(contract) + round-to-5 of (v-35).
// Un-owned talon cards sit in an OPPONENT's pile bits from the start (setup_game),
// so the team pile needs no masking; the rest mask is rebuilt only for :87.
__device__ __forceinline__ u64 score_game(const Game &g) {
    bool klop = g.contract == TK_KLOP;
    u64 p0 = pile_of<0>(g), p1 = pile_of<1>(g), p2 = pile_of<2>(g), p3 = pile_of<3>(g);
    // team pile = the taken cards whose owner seat (B_c A_c) is in the team: per card a 4-way
    // select among the team bits, three bitop3 ("a ? b : c") per half
    u32 t0 = (u32)((int)(g.team << 31) >> 31), t1 = (u32)((int)(g.team << 30) >> 31);
    u32 t2 = (u32)((int)(g.team << 29) >> 31), t3 = (u32)((int)(g.team << 28) >> 31);
    u32 xl = TK_BITOP3(TK_LO(g.A), t1, t0, (a_ & b_) | (~a_ & c_)), yl = TK_BITOP3(TK_LO(g.A), t3, t2, (a_ & b_) | (~a_ & c_));
    u32 xh = TK_BITOP3(TK_HI(g.A), t1, t0, (a_ & b_) | (~a_ & c_)), yh = TK_BITOP3(TK_HI(g.A), t3, t2, (a_ & b_) | (~a_ & c_));
    u32 tl = TK_BITOP3(TK_LO(g.B), yl, xl, (a_ & b_) | (~a_ & c_)) & TK_LO(g.C);
    u32 th = TK_BITOP3(TK_HI(g.B), yh, xh, (a_ & b_) | (~a_ & c_)) & TK_HI(g.C);
    u64 t = TK_U64(tl, th);
    // Navadna_igra.py:87: the declarer plays alone (solo, or called a king of his own) and the
    // called king lies in his pile: the kings are bits 7, 15, 23, 31 of the low word
    u32 kb = g.king * 8 + 7, d = g.declarer;
    bool king_taken = ((TK_LO(g.C) >> kb) & 1) && ((TK_LO(g.A) >> kb) & 1) == (d & 1) && ((TK_LO(g.B) >> kb) & 1) == (d >> 1);
    bool alone_with_king = !klop && g.contract != TK_SOLO_BREZ && __popc(g.team) == 1 && has_king(g.contract) && king_taken;
    if (alone_with_king) t |= talon_unowned(g);
    int c0 = prestej(klop ? p0 : t), c1 = prestej(klop ? p1 : 0), c2 = prestej(klop ? p2 : 0), c3 = prestej(klop ? p3 : 0);
    bool over = c0 > 35 || c1 > 35 || c2 > 35 || c3 > 35;
    int d0 = c0 - 35, ad = d0 < 0 ? -d0 : d0;
    int r = 5 * (int)(((u32)(ad + 2) * 205u) >> 10);                     // int(round(d/5))*5, :103
    if (d0 < 0) r = -r;
    int c = 10 * (int)g.contract;
    int sc = (c0 > 35 ? c : -c) + r;
    int s0 = klop ? (over ? 0 : -c0) : ((g.team & 1) ? sc : 0);
    int s1 = klop ? (over ? 0 : -c1) : ((g.team & 2) ? sc : 0);
    int s2 = klop ? (over ? 0 : -c2) : ((g.team & 4) ? sc : 0);
    int s3 = klop ? (over ? 0 : -c3) : ((g.team & 8) ? sc : 0);
    return pack_scores(s0, s1, s2, s3);
}

// Berac / Odprti_berac at its end (Berac.py:33-44): the declarer took the last trick played (he leads next:
// apply_step has already made the winner the leader) -> -70 / -90, otherwise twelve tricks went by -> +70 / +90.
__device__ __forceinline__ u64 berac_scores(const Game &g) {
    int v = g.contract == TK_BERAC ? 70 : 90;
    int sc = g.leader == g.declarer ? -v : v;
    u32 d = g.declarer;
    return pack_scores(d == 0 ? sc : 0, d == 1 ? sc : 0, d == 2 ? sc : 0, d == 3 ? sc : 0);
}

// One card: the body of krog (Klop.py:47-79, Navadna_igra.py:115-141) after
// igraj_karto returned card `a`, then the per-contract loop bookkeeping
// (Klop.py:27-45, Berac.py:26-44, Navadna_igra.py:72-113).
// Returns 0 = played, 1 = played and the game is finished (scores set),
// -1 = not a legal card: nothing changes except the error bit.
// TRUSTED: `a` was drawn from the legal mask by the in-kernel policy, the membership test
// (Klop.py:57-60, Navadna_igra.py:125-126) cannot fail and is skipped.
// DEFER: a finished game's scores are NOT computed here (scores stays untouched): the caller keeps the
// final state and calls final_scores() on it later (k_play scores the finished games of several tricks
// together, on dense lanes).  want_tv = false skips the trick value (nobody asked for trick_info).
// c_lead: where the caller kept the C plane of the moment the trick's first card was played (the trick-aligned
// card loops), the trick's cards are the bits that plane has gained since; otherwise they come from the ids.
// CARRIED: the caller keeps the game's FamilyWord and the trick's LeadWord (above) and hands them in: the suit led,
// the Berac test and the Klop test are read off them, not rebuilt from g.trick and g.contract.
template <bool TRUSTED = false, bool DEFER = false, bool CARRIED = false>
__device__ __forceinline__ int apply_step(Game &g, u32 a, u64 &scores, u32 &trick_info, bool want_tv = true, const u64 *c_lead = nullptr,
                                          FamilyWord fam = FamilyWord{0u}, LeadWord lead = LeadWord{0u}) {
    if (!TRUSTED) {
        u64 legal = legal_now(g);
        bool ok = a < 54 && ((legal >> (a & 63)) & 1);
        g.error = ok ? g.error : 1u; // (select, not a conditional store: keeps the struct in registers)
        if (!ok) return -1;
    }
    g.C |= 1ULL << a;
    g.trick |= a << (6 * g.nt);
    g.nt++;
    if (g.nt < 4) return 0;
    // pobere_stih / primerjaj_karti (Klop.py:81-94).  The running-best rule there — a challenger wins with a
    // higher card of the best card's suit, or as a tarok against a non-tarok — makes the winner the highest tarok
    // of the trick if one was played, else the highest card of the suit led (a card of any other suit never
    // becomes the best one): read off the trick's card mask instead of three dependent comparisons.
    u64 tm;
    if (c_lead) tm = g.C ^ *c_lead;
    else {
        u32 c0 = g.trick & 63, c1 = (g.trick >> 6) & 63, c2 = (g.trick >> 12) & 63, c3 = (g.trick >> 18) & 63;
        tm = (1ULL << c0) | (1ULL << c1) | (1ULL << c2) | (1ULL << c3);
    }
    // taroks played; cards of the suit led (CARRIED: none where a tarok was led — th is not zero then, and the word is not read)
    u32 th = TK_HI(tm), tl_ = TK_LO(tm) & (CARRIED ? lead.m : (0xFFu << (g.trick & 24)));
    // The winning card is the top bit of the tarok word, or of the suit word when no tarok was played (the card led
    // is a tarok or of its own suit: the chosen word is never zero), and WHO played it is still written in the
    // owner planes at that bit — played cards keep their player's seat bits until the trick changes hands just
    // below.  Word masks, no compares, no selects (see legal_mask).
    u32 zt = tk_zero_mask(th);
    u32 wbit = 31u - (u32)__builtin_clz(TK_BITOP3(th, tl_, zt, (a_ & ~c_) | (b_ & c_)));
    u32 aw = TK_BITOP3(TK_HI(g.A), TK_LO(g.A), zt, (a_ & ~c_) | (b_ & c_)), bw = TK_BITOP3(TK_HI(g.B), TK_LO(g.B), zt, (a_ & ~c_) | (b_ & c_));
    u32 ws = __builtin_amdgcn_ubfe(aw, wbit, 1) | (__builtin_amdgcn_ubfe(bw, wbit, 1) << 1);
    {   // talon gift, Klop.py:67-71: talon.pop() joins the trick after the winner is known
        // 1: a Klop with talon cards left (CARRIED: the Klop bit is the word's top bit, and min(tl, 1) is "cards left")
        u32 gift = CARRIED ? min(g.tl, fam.w >> 31) : (tk_zero_mask(g.contract) & ((g.tl + 7u) >> 3));
        g.tl -= gift;
        u64 gb = 1ULL << ((u32)(g.talon >> (6 * g.tl)) & 63u);
        u32 gm = 0u - gift;
        tm |= TK_U64(TK_LO(gb) & gm, TK_HI(gb) & gm);
    }
    {   // the trick's cards change owner: plane bit := winner's seat bit where tm is set (one bitop3 per half)
        u32 m1 = (u32)((int)(ws << 31) >> 31), m2 = (u32)((int)(ws << 30) >> 31);
        g.A = TK_U64(TK_BITOP3(TK_LO(g.A), TK_LO(tm), m1, (a_ & ~b_) | (b_ & c_)), TK_BITOP3(TK_HI(g.A), TK_HI(tm), m1, (a_ & ~b_) | (b_ & c_)));
        g.B = TK_U64(TK_BITOP3(TK_LO(g.B), TK_LO(tm), m2, (a_ & ~b_) | (b_ & c_)), TK_BITOP3(TK_HI(g.B), TK_HI(tm), m2, (a_ & ~b_) | (b_ & c_)));
    }
    // what rezultat_stiha(stih, sem_pobral) is told (Klop.py:76-77, Navadna_igra.py:138-139):
    // Roka.vrednost_stiha of the 4 (Klop: 5) cards (Roka.py:76-95) and who took them
    if (want_tv) {
        u32 tv = (u32)(popc64(tm) + popc64(tm & (TK_V2 | TK_V3 | TK_V4 | TK_V5)) + popc64(tm & (TK_V3 | TK_V4 | TK_V5)) +
                       popc64(tm & (TK_V4 | TK_V5)) + popc64(tm & TK_V5)) - 2;
        trick_info = 0x8000u | (tv << 4) | ws;
    }
    g.leader = ws; g.nt = 0; g.trick = 0; g.trick_no++;
    // the game is over after twelve tricks, a Berac also the moment the declarer takes a trick (Berac.py:33-39);
    // straight-line selects: lanes of one wave sit in every combination of these cases
    // (as a 0 / 1 number made of plain vector instructions: the caller's test of it is then ONE compare, which a
    // wave vote can use as it is; a vote on a compound condition goes compare -> scalar and -> select -> compare)
    u32 berac01 = CARRIED ? __builtin_amdgcn_ubfe(fam.w, 22u, 1u) : ((0x280u >> g.contract) & 1u);    // TK_BERAC = 7, TK_ODPRTI_BERAC = 9
    u32 over01 = ((g.trick_no + 4u) >> 4) | (berac01 & tk_zero_mask(ws ^ g.declarer));      // (trick_no <= 12)
    if (!DEFER) {
        if (over01) scores = berac01 ? berac_scores(g) : score_game(g);
    }
    g.phase |= over01;                                                   // TK_PHASE_PLAY (2) -> TK_PHASE_DONE (3)
    return (int)over01;
}

// The scores of a game that apply_step has just finished, from its final state alone.
__device__ __forceinline__ u64 final_scores(const Game &g) {
    return (g.contract == TK_BERAC || g.contract == TK_ODPRTI_BERAC) ? berac_scores(g) : score_game(g);
}

// Igra.razdeli's result + engine constructor (Igra.py:38-55,65-73;
// Navadna_igra.py:20-30; Berac.py:15)
__device__ __forceinline__ void setup_game(Game &g, u64 h0, u64 h1, u64 h2, u64 h3, u64 talon36,
                                           u32 contract, u32 declarer, u32 king) {
    g.A = h1 | h3; g.B = h2 | h3;
    g.talon = talon36;
    u64 tal = ids_mask(talon36, 0, 6);
    g.C = tal;
    g.trick = 0; g.nt = 0; g.trick_no = 0; g.error = 0;
    g.contract = contract; g.declarer = declarer;
    g.king = has_king(contract) ? king : 0;
    g.leader = (contract == TK_BERAC || contract == TK_ODPRTI_BERAC) ? declarer : 0;
    if (contract == TK_KLOP) {
        g.team = 0; g.tl = 6;
    } else {
        u32 team = 1u << declarer;
        if (has_king(contract)) {   // partner = holder of the called king BEFORE the exchange
            u64 kb = 1ULL << (king * 8 + 7);
            team |= (h0 & kb) ? 1u : 0u; team |= (h1 & kb) ? 2u : 0u;
            team |= (h2 & kb) ? 4u : 0u; team |= (h3 & kb) ? 8u : 0u;
        }
        g.team = team;
        g.tl = (has_exchange(contract) || contract == TK_SOLO_BREZ) ? 7 : 0;
        // Park the un-owned talon in the pile bits of the lowest seat OUTSIDE the team: whatever
        // of it is never picked up ends with the opponents (Navadna_igra.py:87-92) except in
        // the alone-with-king case, which score_game handles.
        u32 o = (u32)__builtin_ctz(~team & 15u);
        g.A |= (o & 1) ? tal : 0;
        g.B |= (o & 2) ? tal : 0;
    }
    g.phase = has_exchange(contract) ? TK_PHASE_EXCHANGE : TK_PHASE_PLAY;
}

// odpri_talon + menjaj_iz_talona (Navadna_igra.py:36-66, Igralec.py:161-171).
// false = rejected (bad group, card not in hand, duplicate): error bit set.
__device__ __forceinline__ bool apply_exchange(Game &g, u32 choice, u32 d0, u32 d1, u32 d2) {
    u32 gs = group_size(g.contract);
    u32 ngroups = gs == 3 ? 2u : (gs == 2 ? 3u : 6u);
    u64 grp = ids_mask(g.talon, (int)(choice * gs), (int)gs);
    u64 h = hand_of(g, g.declarer) | grp;
    u32 dpk = (d0 & 255) | ((d1 & 255) << 8) | ((d2 & 255) << 16);
    u64 dm = 0;
    bool ok = choice < ngroups;
#pragma unroll
    for (u32 i = 0; i < 3; i++) {
        u32 di = (dpk >> (8 * i)) & 255;
        bool good = di < 54 && ((h >> (di & 63)) & 1) && !((dm >> (di & 63)) & 1);
        ok = ok && (good || i >= gs);
        dm |= (good && i < gs) ? (1ULL << (di & 63)) : 0;
    }
    // all-select update (no conditional stores to different fields: they would push the struct to scratch)
    u32 s = g.declarer;
    u64 nA = (g.A & ~grp) | ((s & 1) ? grp : 0);
    u64 nB = (g.B & ~grp) | ((s & 2) ? grp : 0);
    u64 nC = (g.C & ~grp) | dm;
    g.A = ok ? nA : g.A;
    g.B = ok ? nB : g.B;
    g.C = ok ? nC : g.C;
    g.tl = ok ? choice : g.tl;
    g.phase = ok ? (u32)TK_PHASE_PLAY : g.phase;
    g.error = ok ? g.error : 1u;
    return ok;
}

// ---------------------------------------------------------------------------
// synthetic inputs: counter-based RNG, deal, contract mix, Bot policy
// (the build's own spec; CPU statement in oracle/tarok_spec.py)
// ---------------------------------------------------------------------------
__device__ __forceinline__ u64 mix64(u64 x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27; x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return x;
}
__device__ __forceinline__ u64 game_key(u64 seed, u64 gidx, u64 episode) {
    u64 a = gidx * 0x9E3779B97F4A7C15ULL + episode * 0xD1B54A32D192ED03ULL + 0x2545F4914F6CDD1DULL;
    return mix64(seed ^ mix64(a));
}
// draw i's counter word, premultiplied: a caller that draws i, i + 1, ... carries it and adds TK_RNG_STEP per draw
#define TK_RNG_STEP 0x9E3779B1u
struct RngCtr { u32 v; };
__device__ __forceinline__ RngCtr rng_ctr(u32 i) { return RngCtr{i * TK_RNG_STEP}; }
__device__ __forceinline__ u32 rng32(u32 lo, u32 hi, RngCtr c) {
    u32 x = lo ^ c.v;
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16; x ^= hi;
    x *= 0x27D4EB2Fu; x ^= x >> 15;
    return x;
}
__device__ __forceinline__ u32 rng32(u32 lo, u32 hi, u32 i) { return rng32(lo, hi, rng_ctr(i)); }
__device__ __forceinline__ u32 rng32(u64 key, u32 i) { return rng32((u32)key, (u32)(key >> 32), i); }
__device__ __forceinline__ u32 rng32(u64 key, RngCtr c) { return rng32((u32)key, (u32)(key >> 32), c); }
__device__ __forceinline__ u32 pick(u32 r, u32 n) { return __umulhi(r, n); }

// index of the k-th (0-based) set bit, k < popcount(m): the smallest p with more than k set bits at or below
// it, by bisection on p, one bit of p per level, without a compare or a select (on gfx950 a v_cndmask needs two
// idle slots after the v_cmp that made its mask, and a lone wave pays for them): v_bcnt adds ~k to its count, so
// the sign of the sum says "count <= k", and a funnel shift (v_alignbit) moves that sign into p.
// Per level: v_lshl_or (the candidate), v_bfe (the bits below it), v_bcnt, v_alignbit; 26 instructions in all
// (the bisection that carried the remaining k along and selected on compares: 41).
__device__ __forceinline__ u32 kth_bit(u64 m, u32 k) {
    u32 lo = TK_LO(m), hi = TK_HI(m);
    u32 nk = ~k;                                     // count + nk is negative  <=>  count <= k
    u32 c = (u32)__popc(lo);
    u32 s0 = (u32)((int)(c + nk) >> 31);             // all ones: the bit is in the high word
    u32 w = TK_BITOP3(lo, hi, s0, (a_ & ~c_) | (b_ & c_));
    nk += c & s0;                                    // (~(k - c) = ~k + c)
    u32 p = ((u32)__popc(w & 0xFFFFu) + nk) >> 31;   // p = position / 16
#pragma unroll
    for (int s = 3; s >= 0; s--) {                   // p = position / 2^s after the level
        u32 q = (p << (s + 1)) | (1u << s);
        u32 d = (u32)__popc(__builtin_amdgcn_ubfe(w, 0, q)) + nk;
        p = (p << 1) | (d >> 31);
    }
    return p | (s0 & 32u);
}

// kth_bit for a mask that lies in one word (legal_mask_follow): w = low word | high word, hi_sel = all ones when
// it is the high one.  No first level — nothing to count to tell the words apart; the five levels on w as above.
__device__ __forceinline__ u32 kth_bit_word(u32 w, u32 hi_sel, u32 k) {
    u32 nk = ~k;
    u32 p = ((u32)__popc(w & 0xFFFFu) + nk) >> 31;
#pragma unroll
    for (int s = 3; s >= 0; s--) {
        u32 q = (p << (s + 1)) | (1u << s);
        u32 d = (u32)__popc(__builtin_amdgcn_ubfe(w, 0, q)) + nk;
        p = (p << 1) | (d >> 31);
    }
    return p | (hi_sel & 32u);
}

// uniform card among the legal ones (Bot_igralec.igraj_karto, Igralec.py:158-159)
__device__ __forceinline__ u32 policy_action(u64 key, u32 step, u64 mask) {
    return kth_bit(mask, pick(rng32(key, 128 + step), (u32)popc64(mask)));
}
// the same draw from a follower's one-word mask: one popcount, one-word pick
__device__ __forceinline__ u32 policy_action_follow(u64 key, u32 step, u32 w, u32 hi_sel) {
    return kth_bit_word(w, hi_sel, pick(rng32(key, 128 + step), (u32)__popc(w)));
}

// the same two draws for a caller that carries the counter of card `step`: c = rng_ctr(128 + step)
__device__ __forceinline__ u32 policy_action(u64 key, RngCtr c, u64 mask) {
    return kth_bit(mask, pick(rng32(key, c), (u32)popc64(mask)));
}
__device__ __forceinline__ u32 policy_action_follow(u64 key, RngCtr c, u32 w, u32 hi_sel) {
    return kth_bit_word(w, hi_sel, pick(rng32(key, c), (u32)__popc(w)));
}

// Sequential halving (tarok_playout_cards_halving, include/tarok_env.h): the survivor rule after a round that is not the
// last.  row: a game's [12][4] sums, alive: the ranks that played the round (bits 0..11, every one with the same number of
// playouts behind its sums), seat: the mover.  Of k alive ranks the max(1, ceil(k / 2)) with the highest sum stay, ties
// to the lower rank.  The twelve sums are read once (constant offsets: the reads pipeline, and every lane of a team reads
// the same words, which LDS broadcasts); then `keep` times the best of the ranks left — the highest sum, the lowest rank at
// it — is taken: a rolled loop of at most six passes over twelve registers.  (Rolled loops that re-read LDS for every pair
// cost a launch more than its playouts: every lane of every team runs this; the unrolled 12 x 12 compare table took a
// hundred registers.)  The kernel and tests/host_emu/halving_host.cpp share it.
__device__ __forceinline__ u32 halve_alive(const int *row, u32 alive, u32 seat) {
    int v[12];
#pragma unroll
    for (u32 j = 0; j < 12; j++) v[j] = row[j * 4 + seat];
    u32 rest = alive, out = 0;
#pragma nounroll
    for (u32 n = ((u32)__popc(alive) + 1u) >> 1; n; n--) {
        u32 best = 0;
        int top = 0;
        bool none = true;
#pragma unroll
        for (u32 j = 0; j < 12; j++) {
            const bool up = ((rest >> j) & 1u) && (none || v[j] > top);
            top = up ? v[j] : top;
            best = up ? j : best;
            none = none && !up;
        }
        out |= 1u << best;
        rest &= ~(1u << best);
    }
    return out;
}

// The launch's card among the ranks alive after the last round played: the lowest rank at the maximum of seat's sums
// (12 where none is alive).
__device__ __forceinline__ u32 best_alive(const int *row, u32 alive, u32 seat) {
    u32 best = 12;
    int top = 0;
#pragma unroll
    for (u32 j = 0; j < 12; j++) {
        const int v = row[j * 4 + seat];
        const bool up = ((alive >> j) & 1u) && (best == 12 || v > top);
        top = up ? v : top;
        best = up ? j : best;
    }
    return best;
}

// The compacted item list of tarok_playout_cards_net_halving (include/tarok_env.h): a round's items lie game after game,
// in a game rank after rank of its `on` word, in a rank world after world of the round.  The kernels, the host launcher
// and tests/host_emu/net_halving_host.cpp share these.
//   net_list_slot    the item of the q-th set bit of a game's `on` word in the round's lw-th world (lw = w - e0 < round_worlds)
//   net_list_count   a game's items in the round: the summand of the exclusive prefix sum that gives `base`
//   net_list_alive   a_r, the most ranks a game can have alive in round r: a_0 = 12, a_{r+1} = ceil(a_r / 2) — 12, 6, 3, 2
//   net_list_bound   the round's item bound n * a_r * round_worlds, which sizes the scratch and the play grid
//   net_list_tiles   the play grid: the bound in tiles of `tile` rows, rounded up
#ifdef __HIPCC__
#define TK_HOST_DEVICE __host__ __device__
#else
#define TK_HOST_DEVICE
#endif
TK_HOST_DEVICE __forceinline__ u32 net_list_slot(u32 base, u32 q, u32 round_worlds, u32 lw) { return base + q * round_worlds + lw; }
TK_HOST_DEVICE __forceinline__ u32 net_list_count(u32 on, u32 round_worlds) { return (u32)__builtin_popcount(on) * round_worlds; }
TK_HOST_DEVICE __forceinline__ u32 net_list_alive(u32 round) {
    u32 a = 12;
    for (u32 r = 0; r < round; r++) a = (a + 1u) >> 1;
    return a;
}
TK_HOST_DEVICE __forceinline__ int64_t net_list_bound(int64_t n, u32 round, u32 round_worlds) {
    return n * (int64_t)net_list_alive(round) * (int64_t)round_worlds;
}
TK_HOST_DEVICE __forceinline__ int64_t net_list_tiles(int64_t bound, u32 tile) { return (bound + (int64_t)tile - 1) / (int64_t)tile; }

// The roles of tarok_playout_cards_net_versus (include/tarok_env.h): seats are named RELATIVE to an item's viewer,
// r = (seat - viewer) & 3, and two disjoint 4-bit sets over r say who plays there.  The play kernels, the host's checks and
// tests/host_emu/net_versus_host.cpp share these.
//   net_versus_role        0: the Bot, 1: network A (r in own_rel), 2: network B (r in opp_rel) — the sets are disjoint
//   net_versus_viewer_net  the network whose value head speaks for the viewer at a stop: B if the viewer (r = 0) plays B, else A
//   net_versus_roles_ok    what the entries accept: both sets within 0..15 and no seat in both
TK_HOST_DEVICE __forceinline__ u32 net_versus_role(u32 viewer, u32 mover, u32 own_rel, u32 opp_rel) {
    const u32 r = (mover - viewer) & 3u;
    return ((own_rel >> r) & 1u) | (((opp_rel >> r) & 1u) << 1);
}
TK_HOST_DEVICE __forceinline__ u32 net_versus_viewer_net(u32 opp_rel) { return (opp_rel & 1u) ? 2u : 1u; }
TK_HOST_DEVICE __forceinline__ bool net_versus_roles_ok(int own_rel, int opp_rel) {
    return own_rel >= 0 && own_rel <= 15 && opp_rel >= 0 && opp_rel <= 15 && !(own_rel & opp_rel);
}

// The items of tarok_playout_cards_net_sampled (include/tarok_env.h): a game's slots are (rank j, world w, sample k), sample
// fastest — slot = (j * worlds + w) * samples + k, item = g * slots + slot — so a row's worlds x samples results are
// contiguous for the sum kernel.  The item kernels and tests/host_emu/net_sampled_host.cpp share these.
TK_HOST_DEVICE __forceinline__ u32 net_sampled_slots(u32 worlds, u32 samples) { return 12u * worlds * samples; }
TK_HOST_DEVICE __forceinline__ u32 net_sampled_slot(u32 j, u32 w, u32 k, u32 worlds, u32 samples) { return (j * worlds + w) * samples + k; }
TK_HOST_DEVICE __forceinline__ void net_sampled_split(u32 slot, u32 worlds, u32 samples, u32 &j, u32 &w, u32 &k) {
    const u32 jw = slot / samples;
    k = slot - jw * samples;
    j = jw / worlds;
    w = jw - j * worlds;
}
// the dense item count, or -1 where it reaches 2^31 (the entry's TAROK_EINVAL)
TK_HOST_DEVICE __forceinline__ int64_t net_sampled_items(int64_t n, u32 worlds, u32 samples) {
    const int64_t items = n * (int64_t)net_sampled_slots(worlds, samples);
    return items < (1LL << 31) ? items : -1;
}

// Determinization (tarok_playout_cards_det, include/tarok_env.h): one WORLD of the seat `mover` — the cards it cannot
// see, P = the hands of the three other seats, are dealt afresh among those seats, uniformly over the deals that keep
// the hand sizes.  The cards of P are walked in ascending card number; card i of the walk draws
// r = pick(rng32(wkey, i), cap0 + cap1 + cap2) on the capacities left at that moment and goes to the other seat
// o0 < o1 < o2 whose interval [0, cap0) / [cap0, cap0 + cap1) / the rest r falls into.  Only the A/B planes of P change:
// the mover's hand, the table, the won piles, the talon ids and tl, the contract, the declarer and the called suit stay.
// TEAM: with a called king that lies in P the mover's seat does not know the partner, so the world's team is the
// declarer and whoever received the king; otherwise (king in the mover's hand, played, in the talon, or a contract
// without one) it stays.  A new team moves the un-owned talon cards, which setup_game parked in the pile bits of the
// lowest seat outside the team and score_game counts there, to the lowest seat outside the NEW team.
// Selects only: the one loop runs popcount(P) <= 36 times, the same count on every lane that deals a world of one game.
__device__ __forceinline__ void redeal_unseen(Game &g, u32 mover, u64 wkey) {
    const u32 o0 = mover == 0 ? 1u : 0u, o1 = mover <= 1 ? 2u : 1u, o2 = mover == 3 ? 2u : 3u;
    const u64 h0 = hand_of(g, o0), h1 = hand_of(g, o1), h2 = hand_of(g, o2);
    const u64 P = h0 | h1 | h2;
    u32 cap0 = (u32)popc64(h0), cap1 = (u32)popc64(h1), total = (u32)popc64(P);
    u64 m0 = 0, m1 = 0, rest = P;
    const u32 klo = (u32)wkey, khi = (u32)(wkey >> 32), n = total;
    for (u32 i = 0; i < n; i++) {
        u64 bit = rest & (0ULL - rest);
        u32 r = pick(rng32(klo, khi, i), total);
        u32 t0 = r < cap0 ? 1u : 0u, t1 = (r >= cap0 && r < cap0 + cap1) ? 1u : 0u;
        m0 |= t0 ? bit : 0ULL;
        m1 |= t1 ? bit : 0ULL;
        cap0 -= t0; cap1 -= t1; total--;
        rest ^= bit;
    }
    const u64 m2 = P & ~(m0 | m1);
    u64 sa = ((o0 & 1) ? m0 : 0ULL) | ((o1 & 1) ? m1 : 0ULL) | ((o2 & 1) ? m2 : 0ULL);
    u64 sb = ((o0 & 2) ? m0 : 0ULL) | ((o1 & 2) ? m1 : 0ULL) | ((o2 & 2) ? m2 : 0ULL);
    u64 A = (g.A & ~P) | sa, B = (g.B & ~P) | sb;
    const u64 kb = 1ULL << (g.king * 8 + 7);
    const bool hidden = has_king(g.contract) && (P & kb) != 0;           // the partner is not known at the mover's seat
    const u32 got = (m0 & kb) ? o0 : ((m1 & kb) ? o1 : o2);
    const u32 team = hidden ? ((1u << g.declarer) | (1u << got)) : g.team;
    const u64 un = hidden ? talon_unowned(g) : 0ULL;                     // (a team of a called king: one or two seats)
    const u32 park = (u32)__builtin_ctz((~team & 15u) | 16u);
    g.A = (A & ~un) | ((park & 1) ? un : 0ULL);
    g.B = (B & ~un) | ((park & 2) ? un : 0ULL);
    g.team = team;
}

// The trick leaders of a game replayed from its cards alone (k_observe_ref phase 1, k_shown_voids): nobody stores who
// led trick t.  first_leader: Berac.py:15, Klop.py:26, Navadna_igra.py:70.  next_leader: the seat that led the complete
// trick c0..c3 in, the seat that took it out — pobere_stih (Klop.py:81-94): a challenger beats the best card so far with a
// higher card of its class, or as a tarok against a suit card (class = min(card >> 3, 4): suits 0..3, taroks 4).
__device__ __forceinline__ u32 first_leader(u32 contract, u32 declarer) {
    bool berac = contract == TK_BERAC || contract == TK_ODPRTI_BERAC;
    return berac ? declarer : 0u;
}
__device__ __forceinline__ u32 next_leader(u32 lead, const u32 (&c)[4]) {
    u32 w = 0, cw = c[0];
#pragma unroll
    for (u32 j = 1; j < 4; j++) {
        u32 sw = min(cw >> 3, 4u), si = min(c[j] >> 3, 4u);
        bool beats = (sw == si) ? (cw < c[j]) : (si == 4);
        w = beats ? j : w;
        cw = beats ? c[j] : cw;
    }
    return (lead + w) & 3;
}

// ---------------------------------------------------------------------------------------------------------------------
// Void-aware determinization (tarok_playout_cards_voids, include/tarok_env.h).
// A void word holds bit 5 * seat + class for every (seat, class) the play so far has shown empty (k_shown_voids).
// redeal_voids deals the unseen pool P among the other seats o0 < o1 < o2 uniformly over the deals that keep the hand
// sizes AND give no seat a card of a class it is void in.  Every card of P has an allowed set S of seats: the cards with
// one allowed seat are forced (F_i), those with two form G01, G02, G12, those with three Q.  The number of deals with a
// cards of G01 and b cards of G02 on o0 is
//     T(a, b) = C(n01, a) C(n02, b) C(q, s0) C(n12 + q - s0, r1'),   s0 = r0 - a - b,  r1' = r1 - (n01 - a),
// r_i = c_i - |F_i| (the last factor: how G12 and the rest of Q split between o1 and o2, summed over by Vandermonde).
// (a, b) is drawn in proportion to T from draws 64 and 65 of the world key, and each group is then dealt by the
// sequential form of a uniform subset choice: draw i of the world key for card i of the ascending walk of P (G01, G02
// and Q's share of o0), draw 128 + i for the split of G12 and the rest of Q between o1 and o2.
// Binomials C(n, k), n, k <= 36, from a table in constant memory (k > n reads 0): no run-time-indexed register array.
// The game falls back to redeal_unseen's world — the same draws, hands, team and parking — when the three other seats
// show no void, when a card of P has no allowed seat, when some r_i < 0 or when no consistent deal exists (Total = 0);
// the last three happen only with a void word that is not the game's own.
// Weights are recomputed per world in registers (two passes over (a, b): Total, then the pick): no LDS.
struct TkBinom {
    u64 c[37][37];
    constexpr TkBinom() : c{} {
        for (int n = 0; n < 37; n++)
            for (int k = 0; k <= n; k++) c[n][k] = (k == 0 || k == n) ? 1ULL : c[n - 1][k - 1] + c[n - 1][k];
    }
};
#ifdef __HIPCC__
static __constant__ const TkBinom tk_binom = TkBinom();
__device__ __forceinline__ u64 tk_mulhi64(u64 a, u64 b) { return __umul64hi(a, b); }
#else
static const TkBinom tk_binom = TkBinom();
__device__ __forceinline__ u64 tk_mulhi64(u64 a, u64 b) { return (u64)(((unsigned __int128)a * b) >> 64); }
#endif
// the cards of the classes whose bits are set in v (5 bits: suits 0..3, taroks)
__device__ __forceinline__ u64 class_cards(u32 v) {
    u32 lo = ((v & 1u) ? 0xFFu : 0u) | ((v & 2u) ? 0xFF00u : 0u) | ((v & 4u) ? 0xFF0000u : 0u) | ((v & 8u) ? 0xFF000000u : 0u);
    u32 hi = (v & 16u) ? 0x3FFFFFu : 0u;
    return TK_U64(lo, hi);
}
// T(a, b) as above; 0 outside its support.  All table indices are clamped into the table.
__device__ __forceinline__ u64 voids_weight(u64 c01a, int n02, int n12, int q, int r0, int r1, int r2, int n01, int a, int b) {
    int s0 = r0 - a - b, r1p = r1 - (n01 - a), r2p = r2 - (n02 - b);
    bool ok = s0 >= 0 && s0 <= q && r1p >= 0 && r2p >= 0;
    int s0c = ok ? s0 : 0, r1c = ok ? r1p : 0;
    u64 t = c01a * tk_binom.c[n02][b];
    t *= tk_binom.c[q][s0c];
    t *= tk_binom.c[n12 + q - s0c][r1c];
    return ok ? t : 0ULL;
}
__device__ __forceinline__ void redeal_voids(Game &g, u32 mover, u64 wkey, u32 voids) {
    const u32 o0 = mover == 0 ? 1u : 0u, o1 = mover <= 1 ? 2u : 1u, o2 = mover == 3 ? 2u : 3u;
    const u32 v0 = (voids >> (5 * o0)) & 31u, v1 = (voids >> (5 * o1)) & 31u, v2 = (voids >> (5 * o2)) & 31u;
    const u64 h0 = hand_of(g, o0), h1 = hand_of(g, o1), h2 = hand_of(g, o2);
    const u64 P = h0 | h1 | h2;
    const u64 a0 = P & ~class_cards(v0), a1 = P & ~class_cards(v1), a2 = P & ~class_cards(v2);   // what each seat may hold
    const u64 Q = a0 & a1 & a2, G01 = a0 & a1 & ~a2, G02 = a0 & a2 & ~a1, G12 = a1 & a2 & ~a0;
    const u64 F0 = a0 & ~(a1 | a2), F1 = a1 & ~(a0 | a2), E = P & ~(a0 | a1 | a2);
    const int n01 = popc64(G01), n02 = popc64(G02), n12 = popc64(G12), q = popc64(Q);
    const int r0 = popc64(h0) - popc64(F0), r1 = popc64(h1) - popc64(F1), r2 = popc64(h2) - popc64(a2 & ~(a0 | a1));
    bool plain = (v0 | v1 | v2) == 0 || E != 0 || r0 < 0 || r1 < 0 || r2 < 0 || popc64(P) > 36;  // (36: the table's last row)
    u64 total = 0;
    if (!plain) {
        for (int a = 0; a <= n01; a++) {
            const u64 ca = tk_binom.c[n01][a];
            for (int b = 0; b <= n02; b++) total += voids_weight(ca, n02, n12, q, r0, r1, r2, n01, a, b);
        }
    }
    if (plain || total == 0) { redeal_unseen(g, mover, wkey); return; }
    const u32 klo = (u32)wkey, khi = (u32)(wkey >> 32);
    const u64 u = tk_mulhi64(((u64)rng32(klo, khi, 64u) << 32) | (u64)rng32(klo, khi, 65u), total);
    int sa = 0, sb = 0;
    {   // the first (a, b), a outer and b inner, whose running sum of T exceeds u (u < Total: there is one)
        u64 run = 0;
        bool found = false;
        for (int a = 0; a <= n01; a++) {
            const u64 ca = tk_binom.c[n01][a];
            for (int b = 0; b <= n02; b++) {
                run += voids_weight(ca, n02, n12, q, r0, r1, r2, n01, a, b);
                bool hit = !found && run > u;
                sa = hit ? a : sa; sb = hit ? b : sb;
                found = found || hit;
            }
        }
    }
    // running capacities: G01 (o0, o1), G02 (o0, o2), Q's first stage (o0's share, Q cards left), the o1 / o2 split
    u32 c01a = (u32)sa, c01b = (u32)(n01 - sa), c02a = (u32)sb, c02b = (u32)(n02 - sb);
    u32 k0 = (u32)(r0 - sa - sb), kq = (u32)q, k1 = (u32)(r1 - (n01 - sa)), k2 = (u32)(r2 - (n02 - sb));
    u64 m0 = F0, m1 = F1, rest = P;
    const u32 n = (u32)popc64(P);
    for (u32 i = 0; i < n; i++) {
        const u64 bit = rest & (0ULL - rest);
        const bool g01 = (bit & G01) != 0, g02 = (bit & G02) != 0, g12 = (bit & G12) != 0, inq = (bit & Q) != 0;
        const u32 cap = g01 ? c01a + c01b : (g02 ? c02a + c02b : kq), thr = g01 ? c01a : (g02 ? c02a : k0);
        const bool to0 = (g01 || g02 || inq) && pick(rng32(klo, khi, i), cap) < thr;
        const bool split = g12 || (inq && !to0);                         // the card is o1's or o2's by the second draw
        const bool low = pick(rng32(klo, khi, 128u + i), k1 + k2) < k1;
        const bool to1 = (g01 && !to0) || (split && low);
        m0 |= to0 ? bit : 0ULL;
        m1 |= to1 ? bit : 0ULL;
        c01a -= (g01 && to0) ? 1u : 0u; c01b -= (g01 && !to0) ? 1u : 0u;
        c02a -= (g02 && to0) ? 1u : 0u; c02b -= (g02 && !to0) ? 1u : 0u;
        kq -= inq ? 1u : 0u; k0 -= (inq && to0) ? 1u : 0u;
        k1 -= (split && low) ? 1u : 0u; k2 -= (split && !low) ? 1u : 0u;
        rest ^= bit;
    }
    // the planes, the team of a hidden called king and the re-parked talon: redeal_unseen's
    const u64 m2 = P & ~(m0 | m1);
    u64 pa = ((o0 & 1) ? m0 : 0ULL) | ((o1 & 1) ? m1 : 0ULL) | ((o2 & 1) ? m2 : 0ULL);
    u64 pb = ((o0 & 2) ? m0 : 0ULL) | ((o1 & 2) ? m1 : 0ULL) | ((o2 & 2) ? m2 : 0ULL);
    u64 A = (g.A & ~P) | pa, B = (g.B & ~P) | pb;
    const u64 kb = 1ULL << (g.king * 8 + 7);
    const bool hidden = has_king(g.contract) && (P & kb) != 0;
    const u32 got = (m0 & kb) ? o0 : ((m1 & kb) ? o1 : o2);
    const u32 team = hidden ? ((1u << g.declarer) | (1u << got)) : g.team;
    const u64 un = hidden ? talon_unowned(g) : 0ULL;
    const u32 park = (u32)__builtin_ctz((~team & 15u) | 16u);
    g.A = (A & ~un) | ((park & 1) ? un : 0ULL);
    g.B = (B & ~un) | ((park & 2) ? un : 0ULL);
    g.team = team;
}

// Determinization that also hides what only others have seen (tarok_playout_cards_hidden, include/tarok_env.h): one
// world of the seat `mover` in which, beyond the three other hands,
//   Klop with tl > 0: the tl talon cards nobody has been given yet join the pool, and the pool is dealt to the other
//     seats o0 < o1 < o2 and back into the talon by one ascending walk — card i on draw i of wkey, four running
//     capacities (the hand sizes, tl) — after which the j-th card that landed in the talon, ascending, takes the
//     pick(rng32(wkey, 320 + j), free slots left)-th free slot of slots 0 .. tl - 1.  The ids of those slots, and the A/B/C
//     bits of every card that moved, are rewritten (a Klop's talon card is C = 1, A = B = 0: setup_game);
//   Tri .. Solo_ena after the exchange, mover != declarer: D = the declarer's pile without the cards of the play history
//     (`played`: tarok_played_cards' word) are the discards.  With popcount(D) = group_size and D all discardable, the pool
//     is P' = the three hands | D; D' = a uniform group_size-subset of E = P' & TK_DISCARDABLE by the sequential form
//     (card i of E's ascending walk on draw 256 + i); P' - D' is dealt to o0, o1, o2 by redeal_unseen's walk (draws 0, 1,
//     ..).  D' gets C = 1 and the declarer's A/B bits.  Otherwise the discards stay seen.
// In every other case the pool is redeal_unseen's and so are the draws and the bytes: the one walk below with no talon
// capacity and no discards IS that walk.  Team rule and re-parking: redeal_unseen's (the called king is never
// discardable, so it is in P' - D' exactly when it is in a hand).  Selects only; all trip counts depend on the game alone.
__device__ __forceinline__ void redeal_hidden(Game &g, u32 mover, u64 wkey, u64 played) {
    const u32 o0 = mover == 0 ? 1u : 0u, o1 = mover <= 1 ? 2u : 1u, o2 = mover == 3 ? 2u : 3u;
    const u64 h0 = hand_of(g, o0), h1 = hand_of(g, o1), h2 = hand_of(g, o2);
    const u64 P = h0 | h1 | h2;
    const u32 klo = (u32)wkey, khi = (u32)(wkey >> 32);
    const u32 d = g.declarer, gs = group_size(g.contract);
    // the discards, where they are hidden from the mover
    const u64 dpile = seat_cards(g, d) & g.C & ~played;
    const bool exch = has_exchange(g.contract) && g.tl != 7 && mover != d && (u32)popc64(dpile) == gs && (dpile & ~TK_DISCARDABLE) == 0;
    const u64 D = exch ? dpile : 0ULL;
    u64 Dn = 0;
    {   // D': gs of the cards of E, each taken with probability (still needed) / (cards of E left)
        u64 rest = exch ? ((P | D) & TK_DISCARDABLE) : 0ULL;
        u32 left = (u32)popc64(rest), need = gs;
        const u32 n = left;
        for (u32 i = 0; i < n; i++) {
            u64 bit = rest & (0ULL - rest);
            u32 take = pick(rng32(klo, khi, 256u + i), left) < need ? 1u : 0u;
            Dn |= take ? bit : 0ULL;
            need -= take; left--;
            rest ^= bit;
        }
    }
    // Klop's talon cards that nobody owns yet
    const u32 ntal = g.contract == TK_KLOP ? g.tl : 0u;
    const u64 T = ids_mask(g.talon, 0, (int)ntal);
    const u64 pool = ((P | D) & ~Dn) | T;
    u32 cap0 = (u32)popc64(h0), cap1 = (u32)popc64(h1), cap2 = (u32)popc64(h2), total = cap0 + cap1 + cap2 + ntal;
    u64 m0 = 0, m1 = 0, m2 = 0, rest = pool;
    const u32 n = total;
    for (u32 i = 0; i < n; i++) {
        u64 bit = rest & (0ULL - rest);
        u32 r = pick(rng32(klo, khi, i), total);
        u32 t0 = r < cap0 ? 1u : 0u, t1 = (r >= cap0 && r < cap0 + cap1) ? 1u : 0u;
        u32 t2 = (r >= cap0 + cap1 && r < cap0 + cap1 + cap2) ? 1u : 0u;
        m0 |= t0 ? bit : 0ULL;
        m1 |= t1 ? bit : 0ULL;
        m2 |= t2 ? bit : 0ULL;
        cap0 -= t0; cap1 -= t1; cap2 -= t2; total--;
        rest ^= bit;
    }
    const u64 mT = pool & ~(m0 | m1 | m2);
    {   // the talon's new cards take its free slots 0 .. ntal - 1
        u64 tr = mT, ids = g.talon;
        u32 fm = (1u << ntal) - 1u;
        for (u32 j = 0; j < ntal; j++) {
            u64 bit = tr & (0ULL - tr);
            u32 card = (u32)__builtin_ctzll(bit | (1ULL << 63));
            u32 slot = kth_bit((u64)fm, pick(rng32(klo, khi, 320u + j), (u32)__popc(fm)));
            ids = (ids & ~(63ULL << (6 * slot))) | ((u64)card << (6 * slot));
            fm &= ~(1u << slot);
            tr ^= bit;
        }
        g.talon = ids;
    }
    const u64 U = P | D | T;                                             // every card whose bits may change
    u64 sa = ((o0 & 1) ? m0 : 0ULL) | ((o1 & 1) ? m1 : 0ULL) | ((o2 & 1) ? m2 : 0ULL) | ((d & 1) ? Dn : 0ULL);
    u64 sb = ((o0 & 2) ? m0 : 0ULL) | ((o1 & 2) ? m1 : 0ULL) | ((o2 & 2) ? m2 : 0ULL) | ((d & 2) ? Dn : 0ULL);
    u64 A = (g.A & ~U) | sa, B = (g.B & ~U) | sb;
    g.C = (g.C & ~U) | Dn | mT;
    const u64 kb = 1ULL << (g.king * 8 + 7);
    const bool hidden = has_king(g.contract) && (P & kb) != 0;           // the partner is not known at the mover's seat
    const u32 got = (m0 & kb) ? o0 : ((m1 & kb) ? o1 : o2);
    const u32 team = hidden ? ((1u << d) | (1u << got)) : g.team;
    const u64 un = hidden ? talon_unowned(g) : 0ULL;
    const u32 park = (u32)__builtin_ctz((~team & 15u) | 16u);
    g.A = (A & ~un) | ((park & 1) ? un : 0ULL);
    g.B = (B & ~un) | ((park & 2) ? un : 0ULL);
    g.team = team;
}

// One bidding round between four Bot players (TAROK_MIX_BOT): the control flow of
// Igra.licitacija (Igra.py:75-114) with Bot_igralec.licitiram (Igralec.py:148-152)
// behind the player-side filter (Igralec.py:58-74).  Bids are int(Tip_igre)
// (Naprej -10, Klop 0, Tri 10, Dve 20, Ena 30); the n-th licitiram call of the
// game consumes draw 72 + n.  The re-bidding loop is cut after 8 rounds.
struct BidCtx { u64 key; u32 calls; };
__device__ __forceinline__ int bot_ask(BidCtx &b, int min_igra, int obvezno /* -100 = None */, bool prednost) {
    u32 w = pick(rng32(b.key, 72 + b.calls), 6);
    b.calls++;
    int wish = w < 3 ? -10 : (int)(w - 2) * 10;
    bool ok = prednost ? wish >= min_igra : wish > min_igra;
    return ok ? wish : (obvezno == -100 ? -10 : obvezno);
}
__device__ __forceinline__ void bot_bidding(u64 key, u32 &contract, u32 &declarer) {
    BidCtx b = {key, 0};
    u32 still = 0;
    int top = 10;
#pragma unroll
    for (u32 seat = 1; seat <= 3; seat++) {
        int v = bot_ask(b, top, -100, false);
        if (v != -10) still |= 1u << seat;
        top = max(top, v);
    }
    if (top == 10) {                                 // nobody bid: seat 0 plays at least Klop
        declarer = 0;
        contract = (u32)(bot_ask(b, -10, 0, false) / 10);
        return;
    }
    int v = bot_ask(b, top, -100, true);             // seat 0 may match (priority)
    if (v != -10) still |= 1u;
    top = max(top, v);
    u32 holder = (u32)__builtin_ctz(still);
    for (int rounds = 0; __popc(still) != 1 && rounds < 8; rounds++) {
        u32 nxt = 0;
#pragma unroll
        for (u32 k = 0; k < 4; k++) {
            u32 seat = (k + 1) & 3;                  // 1, 2, 3, 0: seat 0 is asked last
            if ((still >> seat) & 1) {
                v = bot_ask(b, top, seat == holder ? top : -100, false);
                if (v != -10) { nxt |= 1u << seat; holder = seat; top = v; }
            }
        }
        still = nxt;
    }
    declarer = holder;
    contract = (u32)(top / 10);
}

__device__ __forceinline__ void sample_setup(u64 key, int mix, u32 &contract, u32 &declarer, u32 &king) {
    u32 c;
    if (mix == 2) {
        bot_bidding(key, contract, declarer);
        king = has_king(contract) ? pick(rng32(key, 67), 4) : 0;
        return;
    }
    if (mix >= 16) c = (u32)(mix - 16);
    else if (mix == 1) c = TK_TRI + pick(rng32(key, 65), 3);
    else {
        u32 fam = pick(rng32(key, 64), 3), r = rng32(key, 65);
        u32 nav = pick(r, 7);
        u32 navc = nav < 6 ? TK_TRI + nav : TK_SOLO_BREZ;   // Tri,Dve,Ena,Solo_tri,Solo_dve,Solo_ena,Solo_brez
        c = fam == 0 ? TK_KLOP : (fam == 1 ? (pick(r, 2) == 0 ? TK_BERAC : TK_ODPRTI_BERAC) : navc);
    }
    contract = c;
    declarer = c == TK_KLOP ? 0 : pick(rng32(key, 66), 4);
    king = has_king(c) ? pick(rng32(key, 67), 4) : 0;
}

// Bot_igralec.menjaj_iz_talona (Igralec.py:161-171): group 0, random.sample of
// the discardable cards (whole hand if there are too few: the reference raises)
__device__ __forceinline__ void bot_exchange(Game &g, u64 key) {
    u32 gs = group_size(g.contract);
    u64 h = hand_of(g, g.declarer) | ids_mask(g.talon, 0, (int)gs);
    u64 cand = h & TK_DISCARDABLE;
    if ((u32)popc64(cand) < gs) cand = h;
    u32 dpk = 0xFFFFFF;
#pragma unroll
    for (u32 j = 0; j < 3; j++)
        if (j < gs) {
            u32 c = kth_bit(cand, pick(rng32(key, 68 + j), (u32)popc64(cand)));
            dpk = (dpk & ~(255u << (8 * j))) | (c << (8 * j));
            cand &= ~(1ULL << c);
        }
    apply_exchange(g, 0, dpk & 255, (dpk >> 8) & 255, (dpk >> 16) & 255);
}

// The discards of an exchange CANDIDATE (tarok_playout_exchange, include/tarok_env.h): talon group `group` is picked up
// and the Bot's sampler — draws 68 + j of `ckey` on the discardable cards of hand | group, the whole of it if there are
// too few — lays down group_size cards.  Returns them packed, 8 bits each, 255 beyond group_size: what apply_exchange and
// discards_out take.  Under the game's own key and group 0 these are bot_exchange's discards; bot_exchange keeps its own
// copy of the loop so that every kernel that calls it compiles as before.  For a game waiting for the exchange.
__device__ __forceinline__ u32 exchange_discards(const Game &g, u32 group, u64 ckey) {
    u32 gs = group_size(g.contract);
    u64 h = hand_of(g, g.declarer) | ids_mask(g.talon, (int)(group * gs), (int)gs);
    u64 cand = h & TK_DISCARDABLE;
    if ((u32)popc64(cand) < gs) cand = h;
    u32 dpk = 0xFFFFFF;
#pragma unroll
    for (u32 j = 0; j < 3; j++)
        if (j < gs) {
            u32 c = kth_bit(cand, pick(rng32(ckey, 68 + j), (u32)popc64(cand)));
            dpk = (dpk & ~(255u << (8 * j))) | (c << (8 * j));
            cand &= ~(1ULL << c);
        }
    return dpk;
}

// The deal: sort the 54 cards by (random key | card id); position p of the
// sorted order is Igra.razdeli's karte[p] (Igra.py:65-73).
// Per-thread form: 54 keys in registers through a fixed sorting network.
__device__ __forceinline__ void deal_thread(u64 key, u64 &h0, u64 &h1, u64 &h2, u64 &h3, u64 &talon36) {
    u32 a[54];
    u32 lo = (u32)key, hi = (u32)(key >> 32);
#pragma unroll
    for (u32 c = 0; c < 54; c++) a[c] = (rng32(lo, hi, c) & 0xFFFFFFC0u) | c;
#define CS(i, j) { u32 x_ = a[i], y_ = a[j]; a[i] = min(x_, y_); a[j] = max(x_, y_); }
#include "deal_network.inc"
#undef CS
    u64 h[4] = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < 48; p++) h[p / 12] |= 1ULL << (a[p] & 63);
    h0 = h[0]; h1 = h[1]; h2 = h[2]; h3 = h[3];
    u64 t = 0;
#pragma unroll
    for (int p = 0; p < 6; p++) t |= (u64)(a[48 + p] & 63) << (6 * p);
    talon36 = t;
}

// Wave-cooperative form of the same deal for ONE game: lane c holds card c,
// its position is its rank among the 54 keys (54 v_readlane broadcasts), the
// hands fall out of four ballots whose bit index IS the card id.  Must be
// called by all 64 lanes of the wave; klo/khi are wave-uniform.  Used where
// only a few lanes of a wave need a new deal (auto-reset inside a step).
__device__ __forceinline__ void deal_wave(u32 klo, u32 khi, u64 &h0, u64 &h1, u64 &h2, u64 &h3, u64 &talon36) {
    u32 lane = __lane_id();
    u32 key = lane < 54 ? ((rng32(klo, khi, lane) & 0xFFFFFFC0u) | lane) : 0xFFFFFFFFu;
    u32 rank = 0;
#pragma unroll
    for (int j = 0; j < 54; j++) {
        u32 kj = (u32)__builtin_amdgcn_readlane((int)key, j);
        rank += kj < key ? 1u : 0u;
    }
    h0 = __ballot(rank < 12);
    h1 = __ballot(rank >= 12 && rank < 24);
    h2 = __ballot(rank >= 24 && rank < 36);
    h3 = __ballot(rank >= 36 && rank < 48);
    u64 t = 0;
#pragma unroll
    for (u32 p = 0; p < 6; p++) {
        u64 b = __ballot(rank == 48 + p);
        t |= (u64)__builtin_ctzll(b) << (6 * p);
    }
    talon36 = t;
}

// ---------------------------------------------------------------------------
// Playout-valued bidding (tarok_playout_bids / tarok_bid_round, include/tarok_env.h)
// ---------------------------------------------------------------------------
// A viewer's 19 options, one row each: 0 Klop; 1 + 4 (c - 1) + k contract c = Tri, Dve, Ena with suit k called; 13 .. 18
// Solo_tri .. Odprti_berac; row 19 is padding.
#define TK_BID_ROWS 20
#define TK_BID_OPTIONS 19
__device__ __forceinline__ u32 bid_row_contract(u32 r) { return r == 0 ? 0u : (r <= 12 ? 1u + ((r - 1u) >> 2) : r - 9u); }
__device__ __forceinline__ u32 bid_row_king(u32 r) { return (r >= 1 && r <= 12) ? ((r - 1u) & 3u) : 0u; }
// the rows a contract mask (bit code) plays, as a 19-bit word
TK_HOST_DEVICE __forceinline__ u32 bid_row_mask(u32 contracts) {
    u32 m = contracts & 1u;
    m |= (contracts & 2u) ? 0xFu << 1 : 0u;
    m |= (contracts & 4u) ? 0xFu << 5 : 0u;
    m |= (contracts & 8u) ? 0xFu << 9 : 0u;
    return m | (((contracts >> 4) & 0x3Fu) << 13);
}

// The compacted item lists of tarok_playout_exchange_net_list / tarok_playout_bids_net_list (include/tarok_env.h, DESIGN
// §8.22): net_list_slot / net_list_count over UNITS in the place of games.  A unit's `on` word holds its live rows; the
// init, deal and sum kernels, the host's bounds and tests/host_emu/front_list_host.cpp share these statements.
//   exchange: unit g * 6 + i is (game, talon group); its rows are the set indices d < sets of a group the contract has (2
//             groups of three, 3 of two, 6 of one) in a game that takes part — row i * sets + d of the dense launch;
//   bids:     unit g * 4 + v is (game, viewer); its rows are bid_row_mask(contracts), and row 19 with pass_value, for a
//             viewer of the seat set with a valid deal row.
TK_HOST_DEVICE __forceinline__ u32 exchange_list_groups(u32 contract) {
    const u32 gs = 3u - ((contract - 1u) % 3u);          // group_size
    return gs == 3u ? 2u : (gs == 2u ? 3u : 6u);
}
TK_HOST_DEVICE __forceinline__ u32 exchange_list_on(u32 contract, u32 group, u32 sets, bool takes_part) {
    return takes_part && group < exchange_list_groups(contract) ? (1u << sets) - 1u : 0u;
}
TK_HOST_DEVICE __forceinline__ u32 bid_list_rows(u32 contracts, u32 pass_value) {
    return bid_row_mask(contracts) | (pass_value ? 1u << 19 : 0u);
}
TK_HOST_DEVICE __forceinline__ u32 bid_list_on(u32 contracts, u32 pass_value, bool part) { return part ? bid_list_rows(contracts, pass_value) : 0u; }
// The hosts' item bounds: every slot of the exchange's grid (the host cannot read the contracts), and for the bids the
// viewers the seat set can hold (4 with per-game sets) x the rows of `contracts` x the worlds.
TK_HOST_DEVICE __forceinline__ int64_t exchange_list_bound(int64_t n, u32 sets, u32 worlds) { return n * 6 * (int64_t)sets * (int64_t)worlds; }
TK_HOST_DEVICE __forceinline__ int64_t bid_list_bound(int64_t n, u32 seats, bool per_game, u32 contracts, u32 pass_value, u32 worlds) {
    const u32 viewers = per_game ? 4u : (u32)__builtin_popcount(seats & 15u);
    return n * (int64_t)viewers * (int64_t)__builtin_popcount(bid_list_rows(contracts, pass_value)) * (int64_t)worlds;
}

// Sequential halving over those lists (tarok_playout_exchange_net_halving / tarok_playout_bids_net_halving).
// The ARMS are a game's candidates r = i * sets + d (up to 48) or a unit's rows of bid_row_mask (up to 19): bit j of a
// 64-bit `alive` word.  The kernels, the host's bounds and tests/host_emu/front_halving_host.cpp share these statements.
//   front_halving_keep    of k arms alive, max(1, ceil(k / 2)) stay
//   front_halving_stays   the survivor rule as arm j's lane counts it: j stays iff fewer than `keep` alive arms beat it, arm a
//                         beating j when S_a > S_j, or S_a = S_j and a < j — halve_alive's rule (highest sum, ties to the
//                         lower index).  S_a = sums[a * stride]; the sums are re-read from memory (LDS in the kernels) in a
//                         rolled loop over the alive bits: 48 sums are never held in registers (see halve_alive's comment).
//   front_halving_alive   a_r: a_0 = arms, a_{r+1} = ceil(a_r / 2)
//   exchange_halving_bound / bid_halving_bound   the round's item bound B_r
//   front_halving_value   the nearest integer to sum * W / count, halves away from zero, in int64 (0 where count is 0)
TK_HOST_DEVICE __forceinline__ u32 front_halving_keep(u32 k) { return k > 1u ? (k + 1u) >> 1 : 1u; }
TK_HOST_DEVICE __forceinline__ bool front_halving_stays(const int *sums, u32 stride, u64 alive, u32 j) {
    const u32 keep = front_halving_keep((u32)__builtin_popcountll(alive));
    const int sj = sums[j * stride];
    u32 beat = 0;
#pragma nounroll
    for (u64 rest = alive; rest; rest &= rest - 1ULL) {
        const u32 a = (u32)__builtin_ctzll(rest);
        const int sa = sums[a * stride];
        beat += (sa > sj || (sa == sj && a < j)) ? 1u : 0u;
    }
    return beat < keep;
}
TK_HOST_DEVICE __forceinline__ u32 front_halving_alive(u32 arms, u32 round) {
    u32 a = arms;
    for (u32 r = 0; r < round; r++) a = (a + 1u) >> 1;
    return a;
}
TK_HOST_DEVICE __forceinline__ int64_t exchange_halving_bound(int64_t n, u32 sets, u32 round, u32 round_worlds) {
    return n * (int64_t)front_halving_alive(6u * sets, round) * (int64_t)round_worlds;
}
TK_HOST_DEVICE __forceinline__ int64_t bid_halving_bound(int64_t n, u32 seats, bool per_game, u32 contracts, u32 pass_value, u32 round,
                                                        u32 round_worlds) {
    const u32 viewers = per_game ? 4u : (u32)__builtin_popcount(seats & 15u);
    const u32 arms = front_halving_alive((u32)__builtin_popcount(bid_row_mask(contracts)), round) + (pass_value ? 1u : 0u);
    return n * (int64_t)viewers * (int64_t)arms * (int64_t)round_worlds;
}
TK_HOST_DEVICE __forceinline__ int front_halving_value(int sum, int worlds, int count) {
    if (count <= 0) return 0;
    const int64_t num = (int64_t)sum * (int64_t)worlds, mag = num < 0 ? -num : num;
    const int64_t q = (2 * mag + (int64_t)count) / (2 * (int64_t)count);
    return (int)(num < 0 ? -q : q);
}

// World wkey of a bidder: seat `viewer` holds its twelve cards and has seen nothing else, so the other 42 are dealt
// again — redeal_hidden's four-capacity walk (12, 12, 12 and the talon's 6, then the talon's slot order) on the deal set
// up as a Klop, where all six talon cards are un-owned.  The world is (A plane, B plane, talon ids); its C plane is the
// mask of the ids and a talon card has A = B = 0.
__device__ __forceinline__ void bid_world(u64 h0, u64 h1, u64 h2, u64 h3, u64 talon36, u32 viewer, u64 wkey, u64 &A, u64 &B, u64 &ids) {
    Game g;
    setup_game(g, h0, h1, h2, h3, talon36, TK_KLOP, 0, 0);
    g.epar = 0; g.cprev = 0;
    redeal_hidden(g, viewer, wkey, 0ULL);
    A = g.A; B = g.B; ids = g.talon;
}
// The game of row r on a world: the row's contract and king with the viewer as the declarer (Klop: seat 0); partner and
// parking seat by setup_game's own rule on the WORLD's hands.  Left waiting for the exchange where the contract has one.
__device__ __forceinline__ void bid_game(Game &h, u64 A, u64 B, u64 ids, u32 r, u32 viewer) {
    const u64 in_hand = ~ids_mask(ids, 0, 6) & TK_DECK;
    const u32 c = bid_row_contract(r);
    setup_game(h, in_hand & ~A & ~B, in_hand & A & ~B, in_hand & ~A & B, in_hand & A & B, ids, c, c == TK_KLOP ? 0u : viewer, bid_row_king(r));
    h.epar = 0; h.cprev = 0;
}

// The answer of a playout bidder to licitiram(min_igra, obvezno, prednost) from its row of sums S[0 .. 18]: the candidates
// are the rows of the contracts in `contracts` from Tri up that beat (prednost: at least match) min_igra; the best is the
// largest S, the lowest row on ties.  It is bid when S exceeds thr = threshold * playouts and, for a seat that may stand
// on `obvezno` (-100: none), the largest S of that contract's rows; else the seat answers obvezno, or Naprej (-10).
__device__ __forceinline__ int bid_answer(const int32_t *S, int min_igra, int obvezno, bool prednost, long long thr, u32 contracts) {
    int best = -1, bs = 0;
    for (u32 r = 1; r < TK_BID_OPTIONS; r++) {
        const u32 c = bid_row_contract(r);
        const int b = 10 * (int)c, s = S[r];
        const bool cand = ((contracts >> c) & 1u) && (prednost ? b >= min_igra : b > min_igra);
        if (cand && (best < 0 || s > bs)) { best = (int)r; bs = s; }
    }
    bool bid = best >= 0 && (long long)bs > thr;
    if (obvezno != -100) {
        const u32 oc = (u32)(obvezno / 10);
        bool any = false;
        int stand = 0;
        for (u32 r = 0; r < TK_BID_OPTIONS; r++)
            if (bid_row_contract(r) == oc) { stand = (!any || S[r] > stand) ? S[r] : stand; any = true; }
        bid = bid && bs > stand;
    }
    return bid ? 10 * (int)bid_row_contract((u32)best) : (obvezno == -100 ? -10 : obvezno);
}

// One bidding round at a mixed table: bot_bidding's control flow (Igra.licitacija, Igra.py:75-114) with a playout bidder
// on the seats of `set` (sums [4][TK_BID_ROWS], read only for those seats) and the Bot's draw 72 + n elsewhere; every call
// counts in n.  With set = 0 this is sample_setup(key, mix = 2).  The king: the declarer's best row of the contract (the
// lowest suit on ties) for a playout declarer, draw 67 for the Bot, 0 for a contract without one.
struct BidTable { BidCtx b; const int32_t *sums; long long thr; u32 contracts, set; };
__device__ __forceinline__ int bid_ask(BidTable &t, u32 seat, int min_igra, int obvezno, bool prednost) {
    if (!((t.set >> seat) & 1u)) return bot_ask(t.b, min_igra, obvezno, prednost);
    t.b.calls++;
    return bid_answer(t.sums + seat * TK_BID_ROWS, min_igra, obvezno, prednost, t.thr, t.contracts);
}
__device__ __forceinline__ void bid_round(u64 key, const int32_t *sums, int playouts, int threshold, u32 contracts, u32 set,
                                          u32 &contract, u32 &declarer, u32 &king) {
    BidTable t = {{key, 0}, sums, (long long)threshold * (long long)playouts, contracts, set};
    u32 still = 0, holder = 0;
    int top = 10;
    bool open = true;
    for (u32 seat = 1; seat <= 3; seat++) {
        int v = bid_ask(t, seat, top, -100, false);
        if (v != -10) still |= 1u << seat;
        top = max(top, v);
    }
    if (top == 10) {                                 // nobody bid: seat 0 plays at least Klop
        top = bid_ask(t, 0, -10, 0, false);
        open = false;
    }
    if (open) {
        int v = bid_ask(t, 0, top, -100, true);      // seat 0 may match (priority)
        if (v != -10) still |= 1u;
        top = max(top, v);
        holder = (u32)__builtin_ctz(still);
        for (int rounds = 0; __popc(still) != 1 && rounds < 8; rounds++) {
            u32 nxt = 0;
            for (u32 k = 0; k < 4; k++) {
                u32 seat = (k + 1) & 3;              // 1, 2, 3, 0: seat 0 is asked last
                if ((still >> seat) & 1) {
                    v = bid_ask(t, seat, top, seat == holder ? top : -100, false);
                    if (v != -10) { nxt |= 1u << seat; holder = seat; top = v; }
                }
            }
            still = nxt;
        }
    }
    declarer = top == 0 ? 0u : holder;
    contract = (u32)(top / 10);
    u32 kg = 0;
    if (has_king(contract)) {
        if ((set >> declarer) & 1u) {
            const int32_t *S = sums + declarer * TK_BID_ROWS + 1u + 4u * (contract - 1u);
            for (u32 k = 1; k < 4; k++) kg = S[k] > S[kg] ? k : kg;
        } else {
            kg = pick(rng32(key, 67), 4);
        }
    }
    king = kg;
}

// ---------------------------------------------------------------------------
// The bidding head (tarok_bid_values, include/tarok_env.h)
// ---------------------------------------------------------------------------
// The 256 0/1 features of a bidder, seat `seat` holding `hand`, in the policy's layout (feature f = bit f % 64 of word
// f / 64).  Word 0: the hand (bits 0..53), the seat one-hot (54..57).  Word 1: thermometers — bit j (j < 12) iff the hand
// holds more than j taroks, bit 16 + 8k + j (j < 8) iff more than j cards of suit k — then king of suit k held (48 + k)
// and pagat, mond, skis held (52, 53, 54).  Words 2 and 3 are zero (reserved: the layer stays the policy's 256 inputs).
// The kings and the trula are the cards of TK_V5: the suit cards among them, and its lowest, middle and highest tarok.
__device__ __forceinline__ void bid_feature_words(u64 hand, u32 seat, u64 out[4]) {
    constexpr u64 kings = TK_V5 & ~TK_TAROK, trula = TK_V5 & TK_TAROK;
    constexpr u64 skis = 1ULL << (63 - __builtin_clzll(trula)), mond = trula & ~TK_PAGAT & ~skis;
    hand &= TK_DECK;
    const u32 nt = (u32)popc64(hand & TK_TAROK);
    u64 w = (1ULL << (nt < 12u ? nt : 12u)) - 1ULL;
#pragma unroll
    for (u32 k = 0; k < 4; k++) {
        const u64 suit = 0xFFULL << (8 * k);
        w |= ((1ULL << (u32)popc64(hand & suit)) - 1ULL) << (16 + 8 * k);
        w |= (u64)((hand & kings & suit) != 0) << (48 + k);
    }
    w |= (u64)((hand & TK_PAGAT) != 0) << 52;
    w |= (u64)((hand & mond) != 0) << 53;
    w |= (u64)((hand & skis) != 0) << 54;
    out[0] = hand | (1ULL << (54 + (seat & 3u)));
    out[1] = w;
    out[2] = 0;
    out[3] = 0;
}

// ---------------------------------------------------------------------------
// The exchange head (tarok_exchange_values, include/tarok_env.h)
// ---------------------------------------------------------------------------
// The 256 0/1 features of row i, "the declarer picks up talon group i", of a game that waits for the exchange, in the
// policy's layout.  With gs = group_size, d the declarer, H its hand, T the six talon cards, T_i group i and P = H | T_i:
//   word 0  P; bit 54 + d; bits 58, 59, 60: gs = 3, 2, 1; bit 61: a Solo contract.
//   word 1  T & ~T_i (what stays with the opponents); bit 54 + k: the called suit (Tri / Dve / Ena); bit 58 + i.
//   word 2  T_i; bits 54, 55, 56: the called king lies in T_i, in H, in T & ~T_i.
//   word 3  bid_feature_words' word 1 of P — that function's text, called, not restated — with the tarok thermometer
//           carried on to sixteen bits (P holds up to fifteen cards).
// A row the contract does not have (i >= 6 / gs) is four zero words.
__device__ __forceinline__ void exchange_feature_words(const Game &g, u32 i, u64 out[4]) {
    const u32 gs = group_size(g.contract), d = g.declarer;
    const bool live = i * gs < 6u;
    const u64 H = hand_of(g, d), T = talon_all(g), Ti = live ? ids_mask(g.talon, (int)(i * gs), (int)gs) : 0ULL;
    const u64 P = H | Ti, R = T & ~Ti;
    const u64 kb = has_king(g.contract) ? 1ULL << (8 * g.king + 7) : 0ULL;
    const u64 w0 = P | (1ULL << (54 + d)) | (1ULL << (61 - gs)) | ((u64)(g.contract >= TK_SOLO_TRI) << 61);
    const u64 w1 = R | ((kb ? 1ULL : 0ULL) << (54 + g.king)) | ((1ULL << 58) << (i & 7u));
    const u64 w2 = Ti | ((u64)((Ti & kb) != 0) << 54) | ((u64)((H & kb) != 0) << 55) | ((u64)((R & kb) != 0) << 56);
    u64 shape[4];
    bid_feature_words(P, 0u, shape);
    const u32 nt = (u32)popc64(P & TK_TAROK);
    const u64 w3 = shape[1] | ((1ULL << (nt < 16u ? nt : 16u)) - 1ULL);
    out[0] = live ? w0 : 0ULL;
    out[1] = live ? w1 : 0ULL;
    out[2] = live ? w2 : 0ULL;
    out[3] = live ? w3 : 0ULL;
}

// A network output as the exchange head reads it: a NaN counts as -inf (fmaxf returns its other operand), so a broken
// network still yields a valid exchange.  (The builtin: the header needs no <math.h> where g++ compiles it.)
__device__ __forceinline__ float exchange_clean(float y) { return __builtin_fmaxf(y, -__builtin_inff()); }

// The exchange head's discards from one row of 64 outputs: gs times the card of `cand` with the largest clean score, the
// lowest card on ties, removed once taken.  Packed as exchange_discards packs them: 8 bits a card in the order taken, 255
// beyond gs (and where cand runs out, which a candidate mask of an exchange never does).
__device__ __forceinline__ u32 exchange_select(const float *y, u64 cand, u32 gs) {
    u32 dpk = 0xFFFFFFu;
    cand &= TK_DECK;
#pragma unroll
    for (u32 j = 0; j < 3; j++) {
        if (j >= gs) break;
        u32 best = 255u;
        float bv = 0.f;
#pragma unroll
        for (u32 c = 0; c < 54; c++) {
            const float v = exchange_clean(y[c]);
            const bool take = ((cand >> c) & 1ULL) && (best == 255u || v > bv);
            best = take ? c : best;
            bv = take ? v : bv;
        }
        if (best != 255u) {
            dpk = (dpk & ~(255u << (8 * j))) | (best << (8 * j));
            cand &= ~(1ULL << best);
        }
    }
    return dpk;
}

// The exchange head's group from the rows of a game (row i at y + i * stride): the i < ngroups with the largest clean
// output 54, the lowest i on ties.
__device__ __forceinline__ u32 exchange_choice(const float *y, u32 stride, u32 ngroups) {
    u32 best = 0;
    float bv = exchange_clean(y[54]);
#pragma unroll
    for (u32 i = 1; i < 6; i++) {
        const float v = exchange_clean(y[(i < ngroups ? i : 0u) * stride + 54]);
        const bool take = i < ngroups && v > bv;
        best = take ? i : best;
        bv = take ? v : bv;
    }
    return best;
}

// ---------------------------------------------------------------------------
// The value of a pass (tarok_playout_bids_pass / tarok_bid_round_pass, include/tarok_env.h)
// ---------------------------------------------------------------------------
#define TK_BID_PASS_ROW 19
// The bar a bid has to clear at a seat whose row 19 holds the summed score of passing: the pass itself plus `margin`
// points per game.  Stated once: the kernel, the host program and (tests/playout_pass_model.py) the model's own line.
__device__ __forceinline__ long long pass_bar(int s19, int margin, int playouts) {
    return (long long)s19 + (long long)margin * (long long)playouts;
}

// Igra.licitacija's control flow (Igra.py:75-114) once more, as bid_round walks it, with the answers behind
// ask(seat, min_igra, obvezno, prednost); bid_round and bot_bidding keep their own copies so that every kernel that calls
// them compiles as before.  Leaves the final bid and its holder (0 where seat 0 was forced).
template <class Ask> __device__ __forceinline__ void bid_flow(Ask &ask, int &top_out, u32 &holder_out) {
    u32 still = 0, holder = 0;
    int top = 10;
    for (u32 seat = 1; seat <= 3; seat++) {
        int v = ask(seat, top, -100, false);
        if (v != -10) still |= 1u << seat;
        top = max(top, v);
    }
    if (top == 10) {                                 // nobody bid: seat 0 plays at least Klop
        top = ask(0u, -10, 0, false);
    } else {
        int v = ask(0u, top, -100, true);            // seat 0 may match (priority)
        if (v != -10) still |= 1u;
        top = max(top, v);
        holder = (u32)__builtin_ctz(still);
        for (int rounds = 0; __popc(still) != 1 && rounds < 8; rounds++) {
            u32 nxt = 0;
            for (u32 k = 0; k < 4; k++) {
                u32 seat = (k + 1) & 3;              // 1, 2, 3, 0: seat 0 is asked last
                if ((still >> seat) & 1) {
                    v = ask(seat, top, seat == holder ? top : -100, false);
                    if (v != -10) { nxt |= 1u << seat; holder = seat; top = v; }
                }
            }
            still = nxt;
        }
    }
    top_out = top;
    holder_out = top == 0 ? 0u : holder;
}

// The round of a pass playout: three Bots bid under `pkey` (draw 72 + n, every call counted) and seat `viewer` gives its
// least answer on every call — Naprej, or obvezno where it has one (seat 0's forced Klop, the only way it ends as the
// declarer).  The king of a Tri / Dve / Ena is draw 67 of pkey.
struct PassAsk {
    BidCtx b; u32 viewer;
    __device__ __forceinline__ int operator()(u32 seat, int min_igra, int obvezno, bool prednost) {
        if (seat != viewer) return bot_ask(b, min_igra, obvezno, prednost);
        b.calls++;
        return obvezno == -100 ? -10 : obvezno;
    }
};
__device__ __forceinline__ void pass_round(u64 pkey, u32 viewer, u32 &contract, u32 &declarer, u32 &king) {
    PassAsk ask = {{pkey, 0}, viewer};
    int top;
    bid_flow(ask, top, declarer);
    contract = (u32)(top / 10);
    king = has_king(contract) ? pick(rng32(pkey, 67), 4) : 0u;
}

// bid_game with the contract, declarer and king given: the game a pass playout plays on a world.
__device__ __forceinline__ void bid_game_as(Game &h, u64 A, u64 B, u64 ids, u32 contract, u32 declarer, u32 king) {
    const u64 in_hand = ~ids_mask(ids, 0, 6) & TK_DECK;
    setup_game(h, in_hand & ~A & ~B, in_hand & A & ~B, in_hand & ~A & B, in_hand & A & B, ids, contract, declarer, king);
    h.epar = 0; h.cprev = 0;
}

// bid_answer with the seat's own bar: thr = pass_bar(S[19], margin, playouts).  Nothing else of the rule changes.
__device__ __forceinline__ int bid_answer(const int32_t *S, int min_igra, int obvezno, bool prednost, int margin, int playouts,
                                          u32 contracts) {
    return bid_answer(S, min_igra, obvezno, prednost, pass_bar(S[TK_BID_PASS_ROW], margin, playouts), contracts);
}

// bid_round with that answer on the seats of `set` (the trailing tag picks the overload): with row 19 all zero it is
// bid_round at threshold = margin.  The king as there: the declarer's best row, draw 67 for a Bot.
struct BidPassBar {};
struct BidPassAsk {
    BidCtx b; const int32_t *sums; int margin, playouts; u32 contracts, set;
    __device__ __forceinline__ int operator()(u32 seat, int min_igra, int obvezno, bool prednost) {
        if (!((set >> seat) & 1u)) return bot_ask(b, min_igra, obvezno, prednost);
        b.calls++;
        return bid_answer(sums + seat * TK_BID_ROWS, min_igra, obvezno, prednost, margin, playouts, contracts);
    }
};
__device__ __forceinline__ void bid_round(u64 key, const int32_t *sums, int playouts, int margin, u32 contracts, u32 set, BidPassBar,
                                          u32 &contract, u32 &declarer, u32 &king) {
    BidPassAsk ask = {{key, 0}, sums, margin, playouts, contracts, set};
    int top;
    bid_flow(ask, top, declarer);
    contract = (u32)(top / 10);
    u32 kg = 0;
    if (has_king(contract)) {
        if ((set >> declarer) & 1u) {
            const int32_t *S = sums + declarer * TK_BID_ROWS + 1u + 4u * (contract - 1u);
            for (u32 k = 1; k < 4; k++) kg = S[k] > S[kg] ? k : kg;
        } else {
            kg = pick(rng32(key, 67), 4);
        }
    }
    king = kg;
}
