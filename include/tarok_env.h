/* libtarokenv — MI355X-native vectorised Tarok card-play environment, C ABI.
 *
 * Drop-in boundary for ONE hot path of anzeA/Tarok: stepping N independent
 * 4-player games in lock-step — legal-card mask, trick resolution, and
 * Klop / Berac / Navadna_igra scoring.  It replaces what the reference does in
 *
 *     Tarok.paralel_start          Tarok.py:30-62     (N games, 48 lock-steps)
 *     Igra.razdeli + dispatch      Igra.py:38-55,65-73 (deal -> contract engine)
 *     Klop / Berac / Navadna_igra  .start()/.krog()/.mozne_karte()/.pobere_stih()
 *     Roka.prestej                 Roka.py:56-98
 *
 * The reference has no FFI: its "plugin API" is the duck-typed Igralec callback
 * set (Igralec.py:32-122).  Each entry point below names the callback /
 * generator step it stands in for; INTEGRATION.md shows the ctypes binding and
 * the Igralec-protocol adapter (tarok_amd/igralec.py) that sits on top.
 *
 * Conventions
 *   - every function returns int: 0 = OK, negative = TAROK_E*; no exceptions.
 *   - all array arguments are DEVICE pointers owned by the caller (e.g. torch
 *     tensors' data_ptr()), SoA over the env's N games; NULL where allowed.
 *   - `stream` is a hipStream_t (NULL = default stream); every call is
 *     stream-ordered and non-blocking.  One handle per GPU, one host thread per
 *     handle (the reference is single-threaded cooperative generators).
 *   - card id = suit*8 + rank-1 (suits KARA=0 SRCE=1 PIK=2 KRIZ=3), taroks
 *     32..53 (Karta.py:19-23).  Masks are 54-bit sets of card ids.
 *   - contract code = int(Tip_igre)/10 (Tip_igre.py:4-15): 0 Klop, 1 Tri, 2 Dve,
 *     3 Ena, 4 Solo_tri, 5 Solo_dve, 6 Solo_ena, 7 Berac, 8 Solo_brez,
 *     9 Odprti_berac.  Seats are positions in a game's `igralci` list.
 */
#ifndef TAROK_ENV_H
#define TAROK_ENV_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAROK_ABI_VERSION 5
#define TAROK_MAX_CARDS_PER_LAUNCH 192 /* tarok_krog_random / tarok_run_random: cards of every game per launch */
#define TAROK_GAMES_AHEAD 14           /* games every slot keeps dealt ahead for TAROK_AUTO_RESET (tarok_prefetch)  */
#define TAROK_POOL_MAX 64              /* tarok_policy_step_pool: networks in one opponent pool                     */

#define TAROK_OK 0
#define TAROK_EINVAL (-1) /* bad argument                                  */
#define TAROK_EHIP (-2)   /* HIP runtime error: see tarok_last_hip_error() */
#define TAROK_ENOMEM (-3)
#define TAROK_ENODEV (-4) /* no usable GPU                                 */

/* synthetic contract mixes used when tarok_reset gets contract == NULL */
#define TAROK_MIX_ALL 0      /* 1/3 Klop, 1/3 Berac (1/2 open), 1/3 Navadna+Solo over 7 types */
#define TAROK_MIX_NAVADNA3 1 /* Tri / Dve / Ena uniform                                       */
#define TAROK_MIX_BOT 2      /* a bidding round between four Bot players decides (Igra.py:75-114,  */
                             /* Igralec.py:148-156): the reference's own contract distribution    */
#define TAROK_MIX_FIXED 16   /* TAROK_MIX_FIXED + code: every game plays that contract         */

/* flags */
#define TAROK_DEFER_EXCHANGE 1 /* tarok_reset: leave Tri..Solo_ena games waiting for tarok_exchange */
#define TAROK_AUTO_RESET 2     /* step kernels: re-deal a game in the launch that finishes it        */
#define TAROK_CLEAR_COUNTERS 4 /* tarok_reset: also zero the per-slot score sums                     */
#define TAROK_REWARD_REF 8     /* step kernels: reward_out carries what rezultat_igre folds into the last       */
                               /* transition (Igralec.py:421-437): the scores, except that a Berac / Odprti_berac  */
                               /* DEFENDER gets -20 when the hands are empty at the end, else +20               */
#define TAROK_HISTORY 16       /* tarok_create: keep the play history (48 bytes per game), needed by            */
                               /* tarok_observe_ref                                                              */

/* observation word written by tarok_legal_actions / tarok_step (one u64 per game) */
#define TAROK_OBS_MASK ((1ULL << 54) - 1) /* [53:0]  legal-card mask of the seat to move  */
#define TAROK_OBS_SEAT_SHIFT 54           /* [55:54] seat to move                          */
#define TAROK_OBS_STEP_SHIFT 56           /* [61:56] cards played so far in this game      */
#define TAROK_OBS_DONE (1ULL << 62)       /* game finished (step: by this very step)       */
#define TAROK_OBS_ERROR (1ULL << 63)      /* an illegal action was rejected (sticky)       */

/* canonical state lanes of tarok_get_state: lanes_out[lane*N + g] */
#define TAROK_LANE_HAND0 0 /* 0..3  Igralec.roka[id] of seat s                     */
#define TAROK_LANE_PILE0 4 /* 4..7  Igralec.kupcek[id] of seat s                   */
#define TAROK_LANE_TALON 8 /* 6 x 6-bit ordered talon ids (Igra.py:68)             */
#define TAROK_LANE_META 9
#define TAROK_NUM_LANES 10
/* META: [23:0] trick cards 4x6 | [26:24] n_in_trick | [28:27] leader |
 * [32:29] trick_no | [36:33] contract | [38:37] declarer | [41:39] king (7 none) |
 * [45:42] team | [48:46] talon_left | [51:49] chosen group (7 none) |
 * [53:52] phase (1 exchange, 2 play, 3 done) | [54] error                      */

typedef struct tarok_env tarok_env;

const char *tarok_strerror(int code);
int tarok_abi_version(void);
int tarok_device_count(void);      /* number of visible GPUs, 0 if none (never fails) */
int tarok_last_hip_error(void);    /* last hipError_t seen by this library            */

/* One env = n_games slots on one GPU.  game_offset = global index of slot 0
 * (the deal RNG is keyed by seed, game_offset+g and the slot's episode number,
 * so any sharding over GPUs plays identical games).  Replaces building N Igra
 * objects, Tarok.py:33-35.  flags: 0, or TAROK_HISTORY (keep the play history:
 * the `zgodovina` list of Klop.py:63 / Navadna_igra.py:127 as one byte per card). */
int tarok_create(tarok_env **out, int device, int64_t n_games, uint64_t game_offset,
                 uint64_t seed, int mix, int flags);
void tarok_destroy(tarok_env *env);
int64_t tarok_num_games(const tarok_env *env);

/* Launch tuning of an env; the results never depend on it, at whatever point of a run it is changed.  Defaults from the
 * batch size at tarok_create.
 *   TAROK_OPT_REFILL_FAN   1..8 play workgroups whose refill lists one refill workgroup works off.  It sets the step
 *                               launches' grid: changing it after the env's first step launch synchronises the DEVICE,
 *                               restarts the env's launch counters and empties its refill lists (lines whose deal is
 *                               dropped are dealt by their slots when they get there) — do it between phases, not per step,
 *                               and not while a caller's graph holding this env's step launches is to be replayed
 *   TAROK_OPT_LAZY_REFILL  0/1  tarok_step / tarok_step_random: the next-game lines their slots empty are dealt in bulk
 *                               every thirty-second launch instead of in the launch after (default: on below 2^20 games);
 *                               free to change between any two launches */
#define TAROK_OPT_REFILL_FAN 2
#define TAROK_OPT_LAZY_REFILL 3
int tarok_set_option(tarok_env *env, int option, int value);

/* Deal and set up every game: Igra.razdeli (Igra.py:65-73) + the contract
 * engine constructors (Igra.py:38-55; teams Navadna_igra.py:20-30; first
 * leader Klop.py:26 / Berac.py:15 / Navadna_igra.py:70) + the talon exchange
 * (Navadna_igra.py:36-66).  Every slot's episode number is set to `episode`.
 *   deals        [N,54] u8 permutation (hand s = deals[12s:12s+12], talon = deals[48:54]);
 *                NULL = dealt on device by the spec RNG
 *   contract     [N] i8 code; NULL = sampled from the env's mix (then declarer
 *                and king_suit are sampled too)
 *   declarer     [N] i8 seat 0..3 (ignored for Klop); king_suit [N] i8 0..3 (Tri/Dve/Ena)
 *   talon_choice [N] i8 chosen talon group, discards [N,3] u8 (255 pad): what
 *                Igralec.menjaj_iz_talona returns / moves (Igralec.py:161-171);
 *                NULL = the Bot's exchange (group 0, random discardable cards)
 *                unless flags has TAROK_DEFER_EXCHANGE. */
int tarok_reset(tarok_env *env, uint32_t episode, const uint8_t *deals, const int8_t *contract,
                const int8_t *declarer, const int8_t *king_suit, const int8_t *talon_choice,
                const uint8_t *discards, int flags, void *stream);

/* menjaj_iz_talona for the games still waiting for it (Navadna_igra.py:60-66).
 * NULL arrays = the Bot's exchange.  Games not in the exchange phase are untouched. */
int tarok_exchange(tarok_env *env, const int8_t *talon_choice, const uint8_t *discards, void *stream);

/* mozne_karte for the seat to move in every game (Klop.py:96-133,
 * Navadna_igra.py:158-168) = the `mozne` handed to pripravi_igraj_karto.
 * obs_out [N] u64 observation words; seat_out [N] i8 or NULL. */
int tarok_legal_actions(tarok_env *env, uint64_t *obs_out, int8_t *seat_out, void *stream);

/* One card in every unfinished game = one `next(g)` per game at Tarok.py:54:
 * the body of krog (Klop.py:47-79, Navadna_igra.py:115-141) after igraj_karto
 * returned `action`, incl. trick resolution (pobere_stih), the Klop talon gift,
 * Berac's early end and end-of-game scoring.
 *   action     [N] u8 card id.  Not in the legal set -> the game is left
 *              unchanged and its error bit is set (reference: raises Exception,
 *              Klop.py:57-60).  Finished / waiting games ignore it.
 *   reward_out [N,4] i16 scores by seat (`pisejo`): written ONLY for games that
 *              finish in this step; may be NULL
 *   done_out   [N] u8 1 iff the game finished in this step; may be NULL
 *   trick_out  [N] u16, may be NULL: what rezultat_stiha(stih, sem_pobral) is told
 *              (Klop.py:76-77, Navadna_igra.py:138-139).  0 unless this step completed a
 *              trick; then 0x8000 | Roka.vrednost_stiha(stih) << 4 | seat that took it
 *              (Roka.py:76-95; stih = the 4 cards, 5 with Klop's talon card)
 *   obs_out    [N] u64 observation for the NEXT move (see TAROK_OBS_*)
 *   flags      TAROK_AUTO_RESET: a game that finishes is replaced at once by the slot's
 *              next game (episode+1, synthetic contract, Bot exchange, dealt ahead of
 *              time); obs_out then describes the new game and keeps TAROK_OBS_DONE set. */
int tarok_step(tarok_env *env, const uint8_t *action, int16_t *reward_out, uint8_t *done_out,
               uint16_t *trick_out, uint64_t *obs_out, int flags, void *stream);

/* Fill, synchronously, every next-game line that tarok_reset emptied (each slot keeps its next
 * FOURTEEN games dealt ahead: episode+1 .. episode+14, synthetic contract, Bot exchange).  tarok_reset
 * calls it; afterwards the step kernels keep the lines full themselves — a launch that swaps a
 * finished game's successor in puts the replacement deal on a list that extra workgroups of the
 * NEXT step launch work off while that launch plays — so callers normally never need this.  A
 * slot that finds its line missing anyway (more than fourteen games finished within two consecutive
 * launches) deals the game inside the step kernel (same result). */
int tarok_prefetch(tarok_env *env, void *stream);

/* Bot_igralec.igraj_karto (Igralec.py:158-159): uniform choice among the legal
 * cards, drawn from the spec RNG (draw 128 + cards played).  action_out[g] = 255
 * where nothing is to be played. */
int tarok_policy_random(tarok_env *env, const uint64_t *obs, uint8_t *action_out, void *stream);

/* tarok_policy_random + tarok_step fused in one launch; action_out may be NULL. */
int tarok_step_random(tarok_env *env, uint8_t *action_out, int16_t *reward_out, uint8_t *done_out,
                      uint16_t *trick_out, uint64_t *obs_out, int flags, void *stream);

/* `cards` cards of every game in one launch with the Bot policy in-kernel; cards = 4 is one trick,
 * i.e. one pass of the reference's krog generator (Klop.py:47-79, Navadna_igra.py:115-141).
 * The state is read once, kept in registers and written once, but every per-card output is
 * still written: row c (c = 0..cards-1, rows `stride` >= N games apart) of action_out [cards,stride] u8,
 * reward_out [cards,stride,4] i16 (only where done), done_out, trick_out [cards,stride] u16 and
 * obs_out [cards,stride] u64 is what tarok_step_random would have written for the c-th card.
 * action_out / reward_out / done_out / trick_out may be NULL.  Finished games are replaced at
 * once with TAROK_AUTO_RESET (from the slot's dealt-ahead lines; a game can be over after 4 cards,
 * so a slot may start several games inside one launch). */
int tarok_krog_random(tarok_env *env, int cards, int64_t stride, uint8_t *action_out, int16_t *reward_out,
                      uint8_t *done_out, uint16_t *trick_out, uint64_t *obs_out, int flags, void *stream);

/* n_steps lock-steps of the random policy, launched from C (optionally as a
 * replayed hipGraph of `graph_chunk` steps; 0 = eager launches).
 * cards_per_launch = 0: tarok_policy_random + tarok_step per step;  1: tarok_step_random;
 * c >= 2: tarok_krog_random(c) — n_steps, graph_chunk and prefetch_every must be multiples of c
 * and the buffers hold c rows of N (action [c,N], reward_out [c,N,4], done_out [c,N], obs_out [c,N]).
 * prefetch_every = k > 0: an extra tarok_prefetch after every k-th step (graph_chunk must be a
 * multiple of k); normally 0.  Any number of launches per graph: the refill-list parity lives in
 * device memory and is advanced by the launches themselves, so graph replays (this library's or a
 * caller's own capture of tarok_* calls) and eager launches may be mixed in any order.
 * Buffers otherwise as in tarok_step (action [N] u8 scratch is required for cards_per_launch = 0). */
int tarok_run_random(tarok_env *env, int64_t n_steps, int cards_per_launch, int graph_chunk,
                     int prefetch_every, uint8_t *action, int16_t *reward_out, uint8_t *done_out,
                     uint64_t *obs_out, int flags, void *stream);

/* Whole games in one launch (state never leaves registers): deal + setup + Bot
 * exchange + random play to the end, for episode `episode` of every slot.
 *   scores_out [N,4] i16, nsteps_out [N] i16 (cards played; Berac may stop early)
 *   optional step-major traces, [48,N] each, padded with -1 / 0 / 255:
 *   seats_out i8, masks_out u64, actions_out u8.
 * Does not touch the env's stepping state. */
int tarok_rollout_random(tarok_env *env, uint32_t episode, int16_t *scores_out, int16_t *nsteps_out,
                         int8_t *seats_out, uint64_t *masks_out, uint8_t *actions_out, void *stream);

/* Open-hand Monte-Carlo playouts from the env's CURRENT positions: what is each legal card of the seat to move worth?
 * Every legal card is tried and the game played out to its end `samples` times by the Bot (a uniformly random legal card
 * on every seat); the final scores are summed.  The playouts use the TRUE hidden hands — perfect information, no
 * re-dealing of the unseen cards — so the result is an upper-side yardstick and a teacher signal, NOT a fair player.
 *
 * Terms: s = the seat to move, legal = its legal mask, played = trick number * 4 + cards on the table, ep = the slot's
 * episode number, gidx = game_offset + g.  A game TAKES PART iff it is in the play phase and s is in its seat set:
 * `seats`, or seats_per_game[g] & 15 when that array is given (as in tarok_policy_step_seats).
 * For a game that takes part, every rank j < popcount(legal) — c = the j-th lowest legal card — and sample k < samples:
 * copy the game, play c, then play to the end with the Bot: at q cards played the card is the uniform legal card of
 * spec RNG draw 128 + q under the playout key
 *     pkey = game_key(seed ^ salt, gidx, E),   E = 1 << 63 | (u64)ep << 28 | played << 22 | c << 16 | k
 * (bit 63 keeps E apart from every episode number a deal is keyed by), and add the four final scores to
 * sum_out[g][j][0..3].  A card that ends the game outright adds `samples` times that score; a Berac that ends early is
 * scored where it ends.
 *   sum_out     [N,12,4] i32, 16-byte aligned, or NULL.  EVERY row is written: zeros for ranks at or beyond the number
 *               of legal cards and for games that do not take part (a Bot seat to move, a finished game, a game
 *               waiting for the exchange).  sum[j][s] / samples is the card's mean score for the mover.
 *   action_out  [N] u8 or NULL: for a game that takes part the legal card of the smallest rank j that maximises
 *               sum[j][s]; for a game in play whose mover is outside the set the Bot's card (tarok_policy_random's);
 *               255 for any other game.
 * seats = 15: every seat is the Monte-Carlo player; seats = 0: tarok_policy_random's cards, no playout is run.
 * Read-only on the env: the state, the next-game lines and refill lists, the launch counters, the history, the score
 * sums and the play mode are untouched, and the result is a function of the arguments and the state alone.
 * TAROK_EINVAL (before any HIP call) for a NULL env, samples outside 1..TAROK_PLAYOUT_MAX_SAMPLES, seats outside 0..15
 * or both outputs NULL. */
#define TAROK_PLAYOUT_RANKS 12          /* a hand in play never holds more than 12 cards */
#define TAROK_PLAYOUT_MAX_SAMPLES 1024
int tarok_playout_cards(tarok_env *env, int samples, uint64_t salt, int seats, const uint8_t *seats_per_game,
                        int32_t *sum_out, uint8_t *action_out, void *stream);

/* Determinized Monte-Carlo playouts (perfect-information Monte-Carlo over sampled worlds): tarok_playout_cards for a
 * FAIR player.  The playouts of world w run on a uniform re-deal of the cards the seat to move cannot see, so the result
 * is a function of that seat's information set alone: its own hand, the table, the four won piles, the talon ids and
 * `tl`, the contract, the declarer and the called suit.  Terms (s, legal, played, ep, gidx, "takes part", rank j, card
 * c) as above.
 *
 * Unseen pool: P = the union of the hands of the three other seats (the cards with C = 0 that s does not hold).
 * Everything else is the same in every world, and with it the mover's legal cards and their ranks.
 * World w < worlds, under the world key
 *     wkey = game_key(seed ^ salt, gidx, W),   W = 7 << 61 | (u64)ep << 28 | played << 22 | w:
 * let o0 < o1 < o2 be the other seats in seat order and cap_i the size of o_i's true hand.  The cards of P are walked in
 * ascending card number; the i-th card of the walk (i from 0) draws r = pick(rng32(wkey, i), cap0 + cap1 + cap2) on the
 * capacities as they stand at that moment and goes to o0 if r < cap0, to o1 if r < cap0 + cap1, to o2 otherwise; the
 * capacity of the seat that receives it drops by one.  This is uniform over all deals that keep the hand sizes.
 * Team: when the contract has a called king (Tri, Dve, Ena) and the king card 8 * king + 7 lies in P, nobody at s's seat
 * knows the partner, and the world's team is 1 << declarer | 1 << (the seat that received the king).  In every other
 * case — the king in s's hand, played, in the talon, or a contract without one — the team stays.
 * Playouts: in world w, for rank j (card c) and sample k < samples: play c, then the Bot's cards to the end exactly as
 * tarok_playout_cards does (draw 128 + q) under
 *     pkey = game_key(seed ^ salt, gidx, D),   D = 3 << 62 | (u64)ep << 28 | played << 22 | c << 16 | w << 10 | k,
 * and add the four final scores to sum_out[g][j][0..3], taken over all worlds x samples: sum[j][s] / (worlds * samples)
 * is the card's mean score for the mover.  Bits 62 and 61 keep both keys apart from E (bit 63 alone) and from every
 * deal.  World w and sample k depend on neither `worlds` nor `samples`: a launch at (W', S') sums a subset of the
 * playouts of a launch at (W >= W', S >= S').
 * sum_out, action_out, seats / seats_per_game, the games that do not take part and the read-only contract: as for
 * tarok_playout_cards.
 *
 * Known leaks (information the re-deal does not use, or uses though the seat could not have it):
 *   - a void that another seat has shown by not following suit does not constrain the re-deal (it does in
 *     tarok_playout_cards_voids below);
 *   - Klop's face-down talon keeps its true cards in every world;
 *   - the declarer's discards lie in the declarer's pile and so count as seen.
 * TAROK_EINVAL (before any HIP call) for a NULL env, worlds outside 1..TAROK_PLAYOUT_MAX_WORLDS, samples outside
 * 1..TAROK_PLAYOUT_MAX_SAMPLES, seats outside 0..15 or both outputs NULL.  (65,536 playouts of |int16| scores fit the
 * int32 sums.) */
#define TAROK_PLAYOUT_MAX_WORLDS 64
int tarok_playout_cards_det(tarok_env *env, int worlds, int samples, uint64_t salt, int seats, const uint8_t *seats_per_game,
                            int32_t *sum_out, uint8_t *action_out, void *stream);

/* Playout-valued talon exchange: the declarer's one decision before the first card of a Tri, Dve, Ena or Solo contract —
 * which talon group to pick up, which cards to lay down (menjaj_iz_talona: Navadna_igra.py:36-66, Igralec.py:161-171) —
 * valued by determinized playouts.  At this moment the opened talon is shown to the whole table and the discards are
 * the declarer's own, so the only hidden cards are the three other hands: none of tarok_playout_cards_det's leaks
 * applies.  Exact and integer.
 *
 * A game TAKES PART if it waits for the exchange (TAROK_DEFER_EXCHANGE) and its declarer is in the seat set: `seats`,
 * or seats_per_game[g] & 15 when that array is given.  For such a game: gs = the contract's group size (3, 2, 1 for
 * Tri / Solo_tri, Dve / Solo_dve, Ena / Solo_ena), ngroups = 6 / gs, D = discard_sets, ep = the slot's episode, gidx the
 * global game index.
 * Candidate (i, d), i < ngroups, d < D: group i (talon cards i * gs .. i * gs + gs - 1) is picked up and the discards
 * are the Bot's own sampler on the declarer's hand with the group: draws 68 + j, j < gs, of
 *     ckey = game_key(seed ^ salt, gidx, 5 << 61 | (u64)ep << 28 | i << 6 | d),
 * each among the discardable cards left (suit cards below the king, taroks II..VII), among the whole hand if fewer than
 * gs are discardable.  Two candidates may hold the same set; they stay separate candidates.
 * World w < worlds: the three other hands re-dealt by tarok_playout_cards_det's walk with the DECLARER as the viewer, on
 * the game as it waits, under
 *     wkey = game_key(seed ^ salt, gidx, 7 << 61 | (u64)ep << 28 | 63 << 22 | w)
 * (63 in the cards-played field is never a card count: these are not the streams a card launch draws at 0 cards played).
 * The team rule is that launch's: a called king among the three hands makes the world's team the declarer and the seat
 * that received it; with the king in the declarer's hand or in the talon the team stays.  The whole talon, which nobody
 * owns yet, is re-parked with the world's opponents.  The worlds do not depend on the candidate.
 * Playout (i, d, w, k), k < samples: the candidate's exchange is applied to world w and the game played from its first
 * card to the end by the Bot on every seat (draw 128 + q at q cards played) under
 *     pkey = game_key(seed ^ salt, gidx, 3 << 62 | (u64)ep << 28 | 63 << 22 | (8 * i + d) << 16 | w << 10 | k);
 * the four final scores are summed over (w, k) into sum_out[g][i * D + d][0..3].  Key tags, bits 63..61: 101 candidates,
 * 111 worlds, 110 playouts, 100 the open-hand playouts, 000 deals.  Neither d, w nor k depends on the launch's sizes
 * except through the row index: a launch at (W', S', D') sums a corner of one at (W >= W', S >= S', D >= D').
 *   sum_out      [N, 6 * D, 4] i32, 16-byte aligned, or NULL.  EVERY row is written: zeros for groups >= ngroups and
 *                for games that do not take part.
 *   choice_out   [N] i8 and discards_out [N,3] u8 (255 beyond gs), each or NULL, EVERY row written: for a game that
 *                takes part the candidate with the largest sum[declarer], the smallest (i, d) on ties; for a game that
 *                waits with its declarer outside the set exactly the Bot's exchange (group 0, the sampler under the
 *                game's own key: what tarok_exchange does without arrays); -1 and 255, 255, 255 for any other game.
 *                tarok_exchange(choice_out, discards_out) therefore serves a mixed table in one call.
 * Read-only on the env (as tarok_playout_cards), stream-ordered, capturable.
 * TAROK_EINVAL (before any HIP call) for a NULL env, worlds outside 1..TAROK_PLAYOUT_MAX_WORLDS, samples outside
 * 1..TAROK_PLAYOUT_MAX_SAMPLES, discard_sets outside 1..TAROK_EXCHANGE_MAX_SETS or seats outside 0..15.  With all three
 * outputs NULL nothing is launched. */
#define TAROK_EXCHANGE_MAX_SETS 8
#define TAROK_EXCHANGE_ROWS 48          /* 6 groups x TAROK_EXCHANGE_MAX_SETS: the most rows a game's sums can have */
int tarok_playout_exchange(tarok_env *env, int worlds, int samples, int discard_sets, uint64_t salt, int seats,
                           const uint8_t *seats_per_game, int32_t *sum_out, int8_t *choice_out, uint8_t *discards_out, void *stream);

/* Shown voids: what the play so far has told the whole table about who is out of which class of cards.  Needs an env
 * created with TAROK_HISTORY.
 *   voids_out [N] u32, one word per game: bit 5 * seat + class is set iff that seat has shown in this game that it holds
 *   no card of that class; class(card) = min(card >> 3, 4): 0..3 the suits, 4 the taroks (cards 32..53).  Bits 20..31
 *   are 0.  EVERY row is written: 0 for a game that is not in the play phase.
 * Rule, for a game in play with `played` cards so far: history entries 0 .. played - 1 are walked (entries at or beyond
 * `played` are stale and are not read).  Tricks are entries 4t .. 4t + 3; the first leader (the declarer of a Berac, else
 * seat 0) and the winner of every complete trick are replayed from the cards, as tarok_observe_ref replays them.  For
 * card j >= 1 of a trick, complete or on the table, played by seat (lead + j) & 3, with L = the class of the trick's
 * first card and K = the class of this card: if K != L the seat is void in L; if moreover K != 4 and L != 4 it is void in
 * taroks too (it could neither follow suit nor trump; Navadna_igra.py:158-168, Klop.py:96-133).  Klop's talon gift is not
 * a history entry and plays no part.  The rule is sound for every contract: a seat's true hand never holds a card of a
 * class its bits mark void (tests/test_playout_voids_cpu.py plays every contract on the oracle and checks after each card).
 * Read-only on the env, stream-ordered, capturable.
 * TAROK_EINVAL (before any HIP call) for a NULL env or array, or an env without TAROK_HISTORY. */
int tarok_shown_voids(tarok_env *env, uint32_t *voids_out, void *stream);

/* Void-aware determinized playouts: tarok_playout_cards_det whose worlds honour a void word per game.  World w of game g
 * is a re-deal of the unseen pool P that keeps the hand sizes AND gives no other seat a card of a class voids[g] marks it
 * void in, uniform over all such deals, under the SAME world key wkey as tarok_playout_cards_det — but w names another
 * deal than there, unless the game falls back.  The playout keys pkey, the sums, the card rule, "takes part", the
 * read-only contract and the outputs are tarok_playout_cards_det's.  Terms as there: o0 < o1 < o2 the other seats, c_i
 * their true hand sizes.
 *
 * For a card x of P the allowed set is S(x) = { i : bit 5 * o_i + class(x) of the word is clear }; the mover's own bits
 * are ignored.  Groups: F_i = the cards with S = {i} (forced to o_i), G01 / G02 / G12 = those with two allowed seats
 * (sizes n01, n02, n12), Q = those with all three (size q), E = those with none.
 * Fallback: the world is exactly tarok_playout_cards_det's (the same draws, hands, team and parking) when the bits of
 * the three other seats are all zero, when E is not empty, when some r_i = c_i - |F_i| is negative, or when Total below
 * is 0.  The last three arise only with a word that is not the game's own (a hand-built state, a stale history, a
 * caller's array).
 * Counting: for a = 0..n01 (cards of G01 that go to o0) and b = 0..n02 (cards of G02 that go to o0):
 *     s0 = r0 - a - b,  r1' = r1 - (n01 - a),  r2' = r2 - (n02 - b),
 *     T(a, b) = C(n01, a) * C(n02, b) * C(q, s0) * C(n12 + q - s0, r1'),
 * and T(a, b) = 0 unless 0 <= s0 <= q, r1' >= 0, r2' >= 0 (then r1' + r2' = n12 + q - s0).  The last factor sums, by
 * Vandermonde, over how G12 and the rest of Q split between o1 and o2.  T(a, b) is the number of consistent deals with
 * those counts and Total = sum of T the number of all consistent deals; every partial product is a count of partial
 * deals <= 3^36 < 2^58, so 64-bit words hold them.
 * Drawing (a, b): R = (u64)rng32(wkey, 64) << 32 | rng32(wkey, 65), u = the high 64 bits of R * Total; (a, b) is the
 * first pair whose running sum of T exceeds u, a ascending in the outer loop, b ascending in the inner one.  (The pool
 * has at most 36 cards: draws 0..35 and 128..163 are the walks', 64 and 65 are free.)
 * Walks, all in ascending card number; i is the card's index in the ascending walk of ALL of P:
 *   F_i  the card goes to o_i; no draw.
 *   G01  running capacities (capA, capB) = (a, n01 - a): r = pick(rng32(wkey, i), capA + capB); to o0 iff r < capA, else
 *        to o1; the receiver's capacity drops by one.          G02  the same with (b, n02 - b), to o0 or o2.
 *   Q    stage 1, which s0 of its cards go to o0: running (k0, kq) = (s0, q): r = pick(rng32(wkey, i), kq); to o0 iff
 *        r < k0; kq drops at every Q card, k0 when o0 takes the card.
 *   G12 and the Q cards that did not go to o0, as ONE ascending walk: running (k1, k2) = (r1', r2'):
 *        r = pick(rng32(wkey, 128 + i), k1 + k2); to o1 iff r < k1, else to o2.
 * Each stage is the sequential form of a uniform subset choice given (a, b), and (a, b) is drawn in proportion to the
 * number of deals behind it: the world is uniform over the deals that keep the hand sizes and the voids, up to the 2^-64
 * and 2^-32 biases of the two multiply-high picks.  The team of a called king in P is 1 << declarer | 1 << (the seat that
 * received the king), and the un-owned talon is re-parked, as in tarok_playout_cards_det.
 *   voids  [N] u32, required: tarok_shown_voids' words, or any words of the caller's.  With every word 0 both outputs are
 *          byte for byte those of tarok_playout_cards_det.
 * Known leaks left: Klop's face-down talon keeps its true cards in every world; the declarer's discards count as seen.
 * TAROK_EINVAL (before any HIP call) for a NULL env or voids array, worlds outside 1..TAROK_PLAYOUT_MAX_WORLDS, samples
 * outside 1..TAROK_PLAYOUT_MAX_SAMPLES, seats outside 0..15 or both outputs NULL. */
int tarok_playout_cards_voids(tarok_env *env, int worlds, int samples, uint64_t salt, int seats, const uint8_t *seats_per_game,
                              const uint32_t *voids, int32_t *sum_out, uint8_t *action_out, void *stream);

/* The cards of the play history as a set.  Needs an env created with TAROK_HISTORY.
 *   played_out [N] u64, one word per game: bit c is set iff card c is among history entries 0 .. played - 1 of the slot's
 *   current game — every card played so far, the cards of the trick on the table included; a finished game that has not
 *   been re-dealt keeps the cards of its whole play.  Klop's talon gifts and the declarer's discards are not history
 *   entries.  Bits 54..63 are 0.  EVERY row is written: 0 for a game that waits for the exchange, and for a slot whose
 *   finished game has been re-dealt (its new game has played nothing; the stale entries are not read).
 * What it is for: the packed state cannot tell the declarer's discards from the declarer's won tricks; the discards are
 * (the declarer's pile) & ~word.
 * Read-only on the env, stream-ordered, capturable.
 * TAROK_EINVAL (before any HIP call) for a NULL env or array, or an env without TAROK_HISTORY. */
int tarok_played_cards(tarok_env *env, uint64_t *played_out, void *stream);

/* Determinized playouts whose worlds hide what only other seats have seen: tarok_playout_cards_det without its last two
 * leaks.  World w of game g is drawn under the SAME world key wkey as there; the playout keys pkey, the sums, the card
 * rule, "takes part", the read-only contract and the outputs are tarok_playout_cards_det's.  Terms as there: s the seat
 * to move, o0 < o1 < o2 the other seats, cap_i their true hand sizes, P the union of their hands.  Three cases:
 *
 * Klop with tl > 0 talon cards not yet given away (they lie face down in slots 0 .. tl - 1; the winner of the next trick
 *   gets slot tl - 1).  The pool is P plus those tl cards, walked in ascending card number; card i draws
 *   r = pick(rng32(wkey, i), cap0 + cap1 + cap2 + capT) on the capacities left, capT = tl at the start, and goes to o0,
 *   o1, o2 or the talon by the interval r falls into, in that order.  Then the cards that landed in the talon, in
 *   ascending order: the j-th takes the pick(rng32(wkey, 320 + j), free slots left)-th free slot, counted from slot 0,
 *   among slots 0 .. tl - 1.  The world is uniform over the deals that keep the three hand sizes and tl, and over the
 *   orders of the talon's cards.  The ids of slots >= tl (given away, seen) stay.
 * Tri, Dve, Ena, Solo_tri, Solo_dve, Solo_ena in play with s != declarer.  D = (the declarer's pile) & ~played[g]: the
 *   cards the declarer laid down, which only the declarer saw.  If popcount(D) != the contract's group size gs, or D holds
 *   a card that is not discardable (a king, a tarok I, XXI or the skis: the reference lays those down only when the hand
 *   has too few others), the discards stay seen and the world is tarok_playout_cards_det's.  Otherwise the pool is
 *   P' = P | D and E = its discardable cards; D' is a uniform gs-subset of E by the sequential form: E is walked in
 *   ascending card number, card i draws pick(rng32(wkey, 256 + i), cards of E left, this one included) and is taken iff
 *   the draw is below the number still to take.  P' - D' is then dealt to o0, o1, o2 by tarok_playout_cards_det's walk
 *   (draws 0, 1, .. in ascending card order over P' - D', the true hand sizes).  In the world D' lies in the declarer's
 *   pile.  Every D' has the same number of completions, so the world is uniform over all (discards, hands) that keep the
 *   sizes and lay down discardable cards only.
 * Every other game (s == declarer, Klop with tl == 0, Berac, Odprti berac, Solo_brez): the world is exactly
 *   tarok_playout_cards_det's — the same draws, the same bytes of both outputs.
 * Team: as in tarok_playout_cards_det (a called king is never discardable: it is in P' - D' iff it is in P).
 * Draws under a world key: 0..41 the walk, 256..294 the discards, 320..325 the talon slots (the void-aware walk uses
 * 0..35, 64, 65 and 128..163).
 *   played [N] u64, required: tarok_played_cards' words (or the caller's own).
 * Not honoured, by this launch or by tarok_playout_cards_det: the table has seen the picked-up talon group, so those
 * cards are known to be in the declarer's hand or discards; the worlds may deal them to anybody.  That makes the worlds
 * too wide, not too informed.  Shown voids are not combined with this launch.
 * TAROK_EINVAL (before any HIP call) for a NULL env or played array, worlds outside 1..TAROK_PLAYOUT_MAX_WORLDS, samples
 * outside 1..TAROK_PLAYOUT_MAX_SAMPLES, seats outside 0..15 or both outputs NULL. */
int tarok_playout_cards_hidden(tarok_env *env, int worlds, int samples, uint64_t salt, int seats, const uint8_t *seats_per_game,
                               const uint64_t *played, int32_t *sum_out, uint8_t *action_out, void *stream);

/* Playout-valued bidding, part 1: every bid of every seat valued by determinized playouts, BEFORE tarok_reset.  Read-only
 * on the env; the env's games are not read at all.  The game valued is the one tarok_reset(env, episode, deals, ...)
 * would deal: row g of deals [N,54] (validated as tarok_reset validates it; an invalid row gives all-zero sums) or, with
 * deals == NULL, the device's own deal under game_key(seed, gidx, episode), gidx = game_offset + g.
 *
 * Rows (TAROK_BID_ROWS = 20 per viewer): 0 Klop; 1 + 4 (c - 1) + k for contract c = Tri 1, Dve 2, Ena 3 with the king of
 * suit k = 0..3 called (rows 1..12); 13, 14, 15 Solo_tri, Solo_dve, Solo_ena; 16 Berac; 17 Solo_brez; 18 Odprti_berac;
 * 19 reserved, always 0.  A row is played iff bit `code` of `contracts` is set (the contract codes above; int(Tip_igre) /
 * 10); a row that is not played holds 0.
 * Viewers: seat v takes part in game g iff bit v of the seat set is set (`seats`, or seats_per_game[g] & 15).
 * World (v, w), w < worlds: the 42 cards v does not hold are dealt again.  o0 < o1 < o2 the other seats; capacities 12,
 *   12, 12 and 6 for the talon.  The pool is walked in ascending card number; card i draws pick(rng32(wkey, i), cap0 +
 *   cap1 + cap2 + capT) on the capacities as they stand and goes to o0 / o1 / o2 / the talon by its interval.  The talon's
 *   cards then take slots: the j-th of them, ascending, takes the pick(rng32(wkey, 320 + j), free slots left)-th free slot
 *   of 0..5 (tarok_playout_cards_hidden's Klop walk at tl = 6).
 *     wkey = game_key(seed ^ salt, gidx, 2 << 61 | (u64)episode << 28 | v << 6 | w)
 *   Worlds depend on neither the row nor the launch's sizes.
 * Playout (v, r, w, k), k < samples: the game of world w's four hands and talon with the row's contract, declarer v (Klop:
 *   declarer 0) and the row's king; partner and parking seat by the WORLD's hands (a called king in the talon or in v's
 *   hand: v plays alone).  For Tri .. Solo_ena the Bot's exchange under the playout key (group 0, draws 68 + j); then all
 *   cards by the Bot on every seat, draw 128 + q at q cards played; a Berac that ends early is scored where it ends.
 *     pkey = game_key(seed ^ salt, gidx, 3 << 61 | (u64)episode << 28 | v << 26 | r << 21 | w << 15 | k)
 *   The VIEWER's final score is added to sum_out[g][v][r].
 * sum_out [N,4,TAROK_BID_ROWS] i32, 16-byte aligned; EVERY row is written (zeros for seats outside the set, rows outside
 * `contracts` and row 19).  A launch at (W', S') sums a corner of one at (W >= W', S >= S').  With sum_out == NULL nothing
 * is launched.  The first call allocates 40 bytes per game, which the env keeps (not capturable in a graph; later calls
 * are).
 * TAROK_EINVAL (before any HIP call) for a NULL env, worlds outside 1..TAROK_PLAYOUT_MAX_WORLDS, samples outside
 * 1..TAROK_PLAYOUT_MAX_SAMPLES, contracts outside 1..TAROK_BID_ALL_CONTRACTS or seats outside 0..15. */
#define TAROK_BID_ROWS 20
#define TAROK_BID_DEFAULT_CONTRACTS 0x00F /* Klop, Tri, Dve, Ena: the Bot's own range */
#define TAROK_BID_ALL_CONTRACTS 0x3FF
int tarok_playout_bids(tarok_env *env, uint32_t episode, const uint8_t *deals, int worlds, int samples, int contracts, uint64_t salt,
                       int seats, const uint8_t *seats_per_game, int32_t *sum_out, void *stream);

/* Playout-valued bidding, part 2: the bidding round (Igra.licitacija, Igra.py:75-114) of every game on the device, under
 * key = game_key(seed, gidx, episode): seats 1, 2, 3 over a floor of Tri; seat 0's forced call (nobody bid: at least Klop)
 * or priority call; re-bidding rounds with seat 0 asked last and the holder allowed to stand, cut after 8 rounds.  Every
 * call licitiram(seat, min_igra, obvezno, prednost) increments the call counter n.
 * A seat OUTSIDE the set answers as the Bot: draw 72 + n (Naprej 1/2, Tri / Dve / Ena 1/6 each) behind the player-side
 *   filter.
 * A seat v INSIDE the set answers from S(r) = sums[g][v][r] (tarok_playout_bids' rows), bids b = 10 * code:
 *   candidates = the rows of the contracts in `contracts` with b >= 10 and b > min_igra (b >= min_igra with prednost);
 *   best = the candidate with the largest S, the lowest row on ties.
 *   Without obvezno: b(best) if a candidate exists and S(best) > (int64) threshold * playouts, else Naprej.
 *   With obvezno = o: stand = the largest S over the rows of contract o / 10; b(best) if a candidate exists, S(best) > stand
 *   and S(best) > threshold * playouts, else o.
 * contract_out / declarer_out / king_out [N] i8 are what tarok_reset takes, EVERY row written: the final contract, the
 * holder (0 for Klop), and for Tri / Dve / Ena the king: the suit of the declarer's largest S among that contract's four
 * rows (lowest suit on ties) for a declarer in the set, pick(rng32(key, 67), 4) for a Bot declarer; 0 for every other
 * contract.  With seats = 0 and no seats_per_game the outputs are exactly TAROK_MIX_BOT's, and sums may be NULL.
 * TAROK_EINVAL (before any HIP call) for a NULL env, playouts < 1, contracts outside 1..TAROK_BID_ALL_CONTRACTS, seats
 * outside 0..15, sums == NULL with a non-empty set, or all three outputs NULL. */
int tarok_bid_round(tarok_env *env, uint32_t episode, const int32_t *sums, int playouts, int threshold, int contracts, int seats,
                    const uint8_t *seats_per_game, int8_t *contract_out, int8_t *declarer_out, int8_t *king_out, void *stream);

/* The bidding head: a network that writes tarok_playout_bids' array from the twelve cards of each hand, in that launch's
 * place in front of tarok_bid_round.  Read-only on the env; the env's games are not read at all.  The game valued is the
 * one tarok_reset(env, episode, deals, ...) would deal, exactly as tarok_playout_bids defines it (row g of deals, an
 * invalid row giving all-zero rows, or the device's own deal under game_key(seed, gidx, episode)).
 *
 * Row (g, v), v = 0..3, has the 256 0/1 features F(hand of seat v, v), feature f = bit f % 64 of word f / 64:
 *   word 0  bits 0..53 the hand; bit 54 + v (one-hot seat: the seat decides the bidding order, seat 0's forced call and
 *           priority).
 *   word 1  bit j, j < 12: the hand holds more than j taroks; bit 16 + 8 k + j, k < 4, j < 8: more than j cards of suit
 *           k; bit 48 + k: the king of suit k; bits 52, 53, 54: pagat, mond, skis.
 *   words 2, 3  zero (reserved).
 * The row goes through tarok_policy_mlp's network — 256 -> 256 -> 256 -> 64, ReLU, bf16 MFMA with f32 accumulate, both
 * hidden layers stored as bf16 — with w1, b1, w2, b2, w3, b3 in that call's layouts.  Output o < 19 is y of bid row o
 * (the rows of tarok_playout_bids); outputs 19..63 are ignored.
 *   value_out [N,4,TAROK_BID_ROWS] i32, 16-byte aligned, may be NULL:
 *       (int32) rintf(fminf(fmaxf(y * scale, -2^30), 2^30))     (ties to even; a NaN becomes -2^30 by fmaxf)
 *     and 0 for a seat outside the game's set (`seats`, or seats_per_game[g] & 15), a row whose contract bit is not in
 *     `contracts`, row 19 and an invalid deal: tarok_playout_bids' zeros, so the array is interchangeable with its
 *     sum_out as tarok_bid_round's `sums` (playouts then being the caller's own divisor: scale = playouts / the unit
 *     of y in points).  EVERY row is written.
 *   raw_out [N,4,TAROK_BID_ROWS] f32, 16-byte aligned, may be NULL: y before scaling, with the same zeros.
 *   feature_words_out [N,4,4] u64, 16-byte aligned, may be NULL: the four feature words of every seat, in the set or not
 *     (an invalid deal: F(0, v)) — what a learner of the head trains on.
 * Two launches (the deal, then the head); the first call allocates tarok_playout_bids' 40 bytes per game, which the env
 * keeps (not capturable in a graph; later calls are).
 * TAROK_EINVAL (before any HIP call) for a NULL env, weight or bias, a scale that is not finite, <= 0 or > 2^20,
 * contracts outside 1..TAROK_BID_ALL_CONTRACTS, seats outside 0..15 or all three outputs NULL. */
int tarok_bid_values(tarok_env *env, uint32_t episode, const uint8_t *deals, const void *w1, const float *b1, const void *w2,
                     const float *b2, const void *w3, const float *b3, float scale, int contracts, int seats,
                     const uint8_t *seats_per_game, int32_t *value_out, float *raw_out, uint64_t *feature_words_out, void *stream);

/* The value of a pass: what a seat expects to score when ANOTHER seat declares.  Three entries beside tarok_playout_bids,
 * tarok_bid_values and tarok_bid_round, which keep their bytes (row 19 written and read as zero).  Here row
 * TAROK_BID_PASS_ROW = 19 of the [N,4,TAROK_BID_ROWS] array is the pass.  Exact and integer.
 *
 * Pass playout (v, w, k), w < worlds, k < samples, for a viewer v of the game's seat set.  World w of viewer v is
 *   tarok_playout_bids' world, under the same wkey: the pass is valued on the re-deals the nineteen options are valued on.
 *   The playout key is that launch's pkey with r = 19 (it fits the row field's five bits; no other playout uses it):
 *     pkey = game_key(seed ^ salt, gidx, 3 << 61 | (u64)episode << 28 | v << 26 | 19 << 21 | w << 15 | k)
 *   The playout is a TAROK_MIX_BOT game under pkey on the world's hands.  Its bidding round is tarok_bid_round's control
 *   flow (Igra.licitacija) under pkey; every licitiram call counts in n.  The three other seats answer as the Bot does,
 *   draw 72 + n of pkey behind the player-side filter.  Seat v gives its least answer on every call: Naprej, or obvezno
 *   where it has one — seat 0's forced Klop when the three Bots passed, the only way v ends as the declarer.  The king of
 *   a Tri / Dve / Ena is pick(rng32(pkey, 67), 4).  The game is then set up on the WORLD's hands and talon with that
 *   contract, declarer and king: the partner follows from the world, and v may turn out to be the called partner.  The
 *   Bot's exchange (group 0, draws 68 + j of pkey) where the contract has one; every card by the Bot, draw 128 + q at q
 *   cards played.  The VIEWER's final score is added to sum_out[g][v][19].
 *   The three other seats bid as Bots here even where the real table has more seats in the set: row 19 is the seat's
 *   expectation against the Bot's round, not a solution of the bidding game.  It does not depend on `contracts` (a pass is
 *   always an option; the Bots bid in their own range whatever the mask), on the standing bid or on who else is in the set.
 *
 * tarok_playout_bids_pass: tarok_playout_bids' arguments, TAROK_EINVAL conditions and NULL-output rule.  Rows 0..18 of
 *   sum_out are byte for byte tarok_playout_bids' at equal arguments; row 19 is the sum of the worlds * samples pass playouts
 *   of the viewer, 0 for a seat outside the set and for an invalid deal.  A launch at (W', S') sums a corner of one at
 *   (W >= W', S >= S'), row 19 included.
 * tarok_bid_values_pass: tarok_bid_values' arguments, TAROK_EINVAL conditions and outputs.  Rows 0..18 of value_out and
 *   raw_out are byte for byte tarok_bid_values'; row 19 is output 19 of the network, scaled, clamped and rounded as the
 *   other rows are (raw_out: unscaled), 0 for a seat outside the set and for an invalid deal, whatever `contracts` holds.
 * tarok_bid_round_pass: tarok_bid_round with a bar of the seat's own in the constant one's place.  A seat v inside the set
 *   answers by tarok_bid_round's rule with
 *     thr(v) = (int64) S(19) + (int64) margin * playouts
 *   where that rule has threshold * playouts; candidates, the best row, ties, standing on obvezno and the king by the
 *   declarer's best row are unchanged.  `margin` is in points per game, as `threshold` is.  With row 19 all zero the
 *   outputs are tarok_bid_round's at threshold = margin.  tarok_bid_round's TAROK_EINVAL conditions. */
#define TAROK_BID_PASS_ROW 19
int tarok_playout_bids_pass(tarok_env *env, uint32_t episode, const uint8_t *deals, int worlds, int samples, int contracts, uint64_t salt,
                            int seats, const uint8_t *seats_per_game, int32_t *sum_out, void *stream);
int tarok_bid_values_pass(tarok_env *env, uint32_t episode, const uint8_t *deals, const void *w1, const float *b1, const void *w2,
                          const float *b2, const void *w3, const float *b3, float scale, int contracts, int seats,
                          const uint8_t *seats_per_game, int32_t *value_out, float *raw_out, uint64_t *feature_words_out, void *stream);
int tarok_bid_round_pass(tarok_env *env, uint32_t episode, const int32_t *sums, int playouts, int margin, int contracts, int seats,
                         const uint8_t *seats_per_game, int8_t *contract_out, int8_t *declarer_out, int8_t *king_out, void *stream);

/* The exchange head: a network that picks the talon group and the discards, in tarok_playout_exchange's place in front of
 * tarok_exchange.  Read-only on the env, stream-ordered, capturable.  A game TAKES PART exactly as in
 * tarok_playout_exchange: it waits for the exchange (TAROK_DEFER_EXCHANGE) and its declarer is in the seat set (`seats`, or
 * seats_per_game[g] & 15).
 *
 * Notation: gs the group size, ngroups = 6 / gs, d the declarer, H its hand, T the six talon cards, T_i group i (talon
 * cards i gs .. i gs + gs - 1), P_i = H | T_i what the declarer holds after picking group i up.
 * Rows: eight per game, row (g, i), i < 8, "pick up group i"; LIVE iff the game takes part and i < ngroups.  A live row
 * has 256 0/1 features, feature f = bit f % 64 of word f / 64:
 *   word 0  bits 0..53 P_i; bit 54 + d; bits 58, 59, 60: gs = 3, 2, 1; bit 61: the contract is a Solo.
 *   word 1  bits 0..53 T & ~T_i (what stays with the opponents); bit 54 + k: called-king suit k (Tri / Dve / Ena only);
 *           bit 58 + i.
 *   word 2  bits 0..53 T_i; bits 54, 55, 56: the called king lies in T_i, in H, in T & ~T_i (Tri / Dve / Ena only).
 *   word 3  on P_i: bit j, j < 16: more than j taroks; bit 16 + 8 k + j, j < 8: more than j cards of suit k; bit 48 + k:
 *           the king of suit k; bits 52, 53, 54: pagat, mond, skis (tarok_bid_values' word 1 with sixteen tarok bits).
 * A row that is not live has four zero words.
 * The row goes through tarok_policy_mlp's network — 256 -> 256 -> 256 -> 64, ReLU, bf16 MFMA with f32 accumulate, both
 * hidden layers stored as bf16 — with w1 .. b3 in that call's layouts.  Output c < 54 is the discard score of card c,
 * output 54 the value of the group (the policy's own layout: 54 logits and the value column); 55..63 are ignored.
 * clean(y) = fmaxf(y, -inf): a NaN becomes -inf, so a broken network still yields a valid exchange.
 * The decision of a game that takes part:
 *   choice    i* = the i < ngroups with the largest clean(y_i[54]), the lowest i on ties;
 *   cand      P_i* & the discardable cards (suit ranks 1..7 and taroks 2..7, as for the Bot), all of P_i* if those
 *             are fewer than gs: the Bot's own rule;
 *   discards  gs times the card of cand with the largest clean(y_i*[c]), the lowest card on ties, removed once taken.
 * Outputs, each may be NULL, EVERY row written:
 *   raw_out [N,8,64] f32, 16-byte aligned: the 64 outputs of a live row, zeros for every other row.
 *   choice_out [N] i8, discards_out [N,3] u8 (255 beyond gs, the cards in the order taken): tarok_playout_exchange's three
 *     cases — the decision above; the Bot's exchange (group 0, its sampler under the game's own key) for a game that
 *     waits with its declarer outside the set; -1 and 255, 255, 255 for any other game — so tarok_exchange(choice_out,
 *     discards_out) serves a mixed table in one call.
 *   feature_words_out [N,8,4] u64, 16-byte aligned: the four words of every row (zero where not live) — what a learner
 *     of the head trains on.
 * With all four outputs NULL nothing is launched.
 * TAROK_EINVAL (before any HIP call) for a NULL env, weight or bias, or seats outside 0..15. */
int tarok_exchange_values(tarok_env *env, const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                          const float *b3, int seats, const uint8_t *seats_per_game, float *raw_out, int8_t *choice_out,
                          uint8_t *discards_out, uint64_t *feature_words_out, void *stream);

/* What tarok_playout_exchange's candidates laid down: its sum_out says what candidate (i, d) was worth, this launch which
 * cards it discarded — what a learner of the exchange head's discard scores needs.  Read-only, stream-ordered.
 *   cand_out [N, 6 * discard_sets, 3] u8: row i * discard_sets + d holds the discards of group i under
 *     ckey = game_key(seed ^ salt, gidx, 5 << 61 | (u64)episode << 28 | i << 6 | d), tarok_playout_exchange's to the bit,
 *     255 beyond gs; 255, 255, 255 for groups >= ngroups and for games that do not take part.  EVERY row is written.
 * With cand_out == NULL nothing is launched.  TAROK_EINVAL (before any HIP call) for a NULL env, discard_sets outside
 * 1..TAROK_EXCHANGE_MAX_SETS or seats outside 0..15. */
int tarok_exchange_candidates(tarok_env *env, int discard_sets, uint64_t salt, int seats, const uint8_t *seats_per_game,
                              uint8_t *cand_out, void *stream);

/* The bid and exchange heads on the games TAROK_AUTO_RESET deals ahead.  A slot keeps its next
 * TAROK_GAMES_AHEAD games in next-game lines, each dealt, bid (the Bot's round of the env's mix) and exchanged (the Bot's)
 * by a refill.  This call decides the front of every such game again that has not been fronted yet, in the lines, between
 * two step launches: stream-ordered, capturable, nothing allocated, no host read.
 *   Lines taken.  Line b of slot j (j < N) iff its episode tag nep lies in (episode[j], episode[j] + TAROK_GAMES_AHEAD] with
 *     nep % TAROK_GAMES_AHEAD == b — the line is valid now, not one waiting on a refill list — and its front mark (a u32
 *     at byte 44 of the 64-byte line, which no step kernel reads and no deal writes) differs from nep.  tarok_reset clears
 *     the marks; a line dealt again carries another episode.
 *   What is written, with key = game_key(seed, offset + j, nep) (the line's own key):
 *     the deal of key;
 *     with bid weights: the round of tarok_bid_round (pass_value != 0: tarok_bid_round_pass) under key, whose seats in
 *       the slot's set (seats, or seats_per_game[j] & 15) answer from tarok_bid_values[_pass]' values of that deal at
 *       (scale, contracts), held against threshold (margin) `margin` at `playouts`; the other seats are Bots.  Without:
 *       the env's mix under key, as the line had it;
 *     the game set up for episode nep;
 *     where the contract has an exchange: with exchange weights and the declarer in the set, tarok_exchange_values'
 *       choice and discards, applied; else the Bot's exchange under key;
 *     the line's two packed pairs, and the mark = nep.  Key and tag keep their bytes.
 *   With the empty set (seats = 0, no seats_per_game) every line taken keeps its first 44 bytes and gains the mark.
 *   A line on a pending refill list has a stale tag and is skipped: the refill deals it unfronted, the next call takes it.
 *   A slot that runs out of lines deals in place, the Bot's front.  With one-card launches (tarok_policy_step*) a line
 *   dealt after a call belongs to a game at least thirteen games ahead: a call every 48 launches or oftener leaves no game
 *   to start unfronted.
 *   count_out [1] i64 (device, may be NULL): the lines this call fronted; contract_hist_out [10] i64 (device, may be
 *   NULL): their contracts.  scratch: tarok_front_lines_scratch_bytes(N) bytes of device memory, 16-byte aligned, contents
 *   irrelevant before and after (8-byte items behind a 128-byte header: the lines taken, compacted; the count stays on
 *   the device).  Up to five launches.
 * TAROK_EINVAL (before any HIP call) for a NULL env, a weight set given in part, both sets NULL, bid weights with scale
 * outside (0, 2^20], playouts < 1, contracts outside 1..TAROK_BID_ALL_CONTRACTS or an env whose mix is not TAROK_MIX_BOT
 * (the exchange weights alone go with any mix), seats outside 0..15, scratch NULL or scratch_bytes too small. */
int64_t tarok_front_lines_scratch_bytes(int64_t n_games);
int tarok_front_lines(tarok_env *env, const void *bid_w1, const float *bid_b1, const void *bid_w2, const float *bid_b2,
                      const void *bid_w3, const float *bid_b3, float scale, int playouts, int margin, int contracts,
                      int pass_value, const void *exchange_w1, const float *exchange_b1, const void *exchange_w2,
                      const float *exchange_b2, const void *exchange_w3, const float *exchange_b3, int seats,
                      const uint8_t *seats_per_game, void *scratch, int64_t scratch_bytes, int64_t *count_out,
                      int64_t *contract_hist_out, void *stream);

/* The next-game lines as they stand: what the tests of tarok_front_lines compare and what a checkpoint of a fronted env
 * holds beside tarok_get_state.  Read-only, stream-ordered; either output may be NULL.
 *   lines_out [N, TAROK_GAMES_AHEAD, 6] u64: the line's four packed words, its key, and nep | (u64)mark << 32.
 *   lanes_out [10, N * TAROK_GAMES_AHEAD] u64: the line's game as tarok_get_state's lanes (line t = j * TAROK_GAMES_AHEAD + b);
 *     meaningful for a line whose tag is valid. */
int tarok_get_lines(tarok_env *env, uint64_t *lines_out, uint64_t *lanes_out, void *stream);

/* A playout launch's sums as a teacher's target distribution: one row of 64 bf16 per game, for the learner's distillation
 * term (tarok_learn_chain_distill).  Per game g the kernel reads obs[g], the observation word the playouts started from:
 * legal = its 54-bit mask, s = its seat bits, nl = min(popcount(legal), TAROK_PLAYOUT_RANKS).
 * The game HAS A TEACHER iff legal != 0 and s is in the game's seat set (`seats`, or seats_per_game[g] & 15 when that array
 * is given, exactly as in tarok_playout_cards).  On the words the env writes this is the playout launches' "takes part":
 * a word carries legal cards iff its game is in the play phase (a finished game without TAROK_AUTO_RESET and a game
 * waiting for the exchange have legal = 0).  TAROK_OBS_DONE and TAROK_OBS_ERROR are NOT part of the rule, because they do
 * not tell such games apart: with TAROK_AUTO_RESET the word that describes a slot's NEXT game keeps TAROK_OBS_DONE (the
 * first card of every game of a rollout), and the error bit is sticky while its game plays on — the playout launches play
 * both, and both get their teacher's row.  The word tells every case apart; nothing else is passed.
 *   with a teacher:  z_j = (sums[g][j][s] - max_k sums[g][k][s]) / (playouts * tau) for the ranks j, k < nl (the difference
 *                    in integers, the rest in float32; the divisor is the float32 product), and
 *                    target[g][c] = bf16(exp(z_j) / sum_k exp(z_k)), round to nearest even, at the j-th lowest legal card
 *                    c; 0 in every other column 0..63.  tau = 0: 1.0 at the card of the smallest rank that maximises
 *                    sums[g][j][s] — the card action_out of the playout launch names — and 0 elsewhere.
 *   without:         all 64 columns 0.
 * EVERY row is written.  Nothing of the env is read but its size and device: the result is a function of the arguments.
 * sums [N,12,4] i32 (16-byte aligned), obs [N] u64, playouts = the playouts behind every sum (samples, or worlds *
 * samples), target_out [N,64] bf16 (16-byte aligned).
 * TAROK_EINVAL (before any HIP call) for a NULL env or array (seats_per_game may be NULL), playouts < 1, tau < 0, NaN or
 * infinite, a tau > 0 whose float32 product playouts * tau overflows or is not a normal number (below 2^-126), seats
 * outside 0..15. */
int tarok_playout_targets(tarok_env *env, const int32_t *sums, const uint64_t *obs, int playouts, float tau, int seats,
                          const uint8_t *seats_per_game, void *target_out, void *stream);

/* Observation features of the seat to move for a policy network: features_out [N,256] bf16,
 * every entry 0.0 or 1.0 (feature set documented at k_observe — the build's own,
 * the reference's encoder is part of its LSTM agent, Igralec.py:453-543):
 *   [0,54) own hand, [54,64) contract one-hot;  [64,118) legal cards, [118,128) declarer
 *   relative seat (4) / cards on table count (4) / on declarer's team / contract calls a king;
 *   [128,182) cards on the table, [182,192) called-king suit (4) / trick number binary (4);
 *   [192,246) cards already taken, [246] game live.
 * The seat to move is (leader + cards on the table) % 4.  "Cards already taken" are the four piles: every seat's won
 * tricks, Klop's gifted talon cards with the trick they went to, and the declarer's discards; talon cards that lie in
 * nobody's pile (the groups not picked up, Klop's talon not yet gifted) are in no region.
 * For a game that is NOT in play — waiting for the exchange (TAROK_DEFER_EXCHANGE) or finished without an auto-reset —
 * the legal region and the live bit are 0 and every other region is what the game's state holds: for a waiting game
 * the twelve dealt cards of seat 0, an empty table, trick number 0 and no card taken; for a finished game the cards
 * left in the hand of the seat that took the last trick (none after twelve tricks), an empty table, the trick number
 * at which it ended (12, or lower for a Berac lost earlier) and every pile.  The rows of such games are written like
 * any other.  tests/observe_model.py states all of this on the CPU oracle; tests/test_gpu_observe_features.py holds
 * tarok_observe and the fused policy launches' features_out / feature_words_out to it bit for bit. */
#define TAROK_OBS_FEATURES 256
int tarok_observe(tarok_env *env, void *features_out, void *stream);

/* ---- the reference's own observation layout (parity unpinned: the reference holds no
 * fixture for it and Igralec.py cannot be imported — tested against the line-cited restatement
 * oracle/encoder_spec.py).  Needs an env created with TAROK_HISTORY.
 *
 * tarok_observe_ref: what Nevronski_igralec.stanje_v_vektor_rek_navadna (Igralec.py:453-533) builds
 * for the seat to move of every game in play, as ONE record of 0/1 bytes per game:
 *   record_out [N, TAROK_REF_RECORD_BYTES] u8, fields at the byte offsets below (row-major):
 *     TAROK_REF_OPP      [56][3][54]  input_layer_nasprotiki: row i = the i-th card played in the game, one-hot
 *                                     card in the channel of the opponent who played it (the other three
 *                                     seats in seat order, Igralec.py:271-274); own plays leave the row empty
 *     TAROK_REF_OWN      [56][54]     roka_input: row i of an own play = the hand vector before that card; it
 *                                     starts from the hand as dealt (zacetna_roka; the exchange is not applied)
 *     TAROK_REF_TALON    [6][55]      talon_input of Tri..Solo_ena (row r: the r-th talon card, column 54: in the
 *                                     chosen group; all zero for Solo_brez); for Klop the first 54 bytes are its
 *                                     flat talon vector (the cards gifted so far); zero for Berac
 *     TAROK_REF_KING     [4]          barva_kralja one-hot (Tri/Dve/Ena)
 *     TAROK_REF_INDEX    [4]          index_tistega_ki_igra one-hot: the declarer among the other seats in seat
 *                                     order, 3 = the mover himself
 *     TAROK_REF_DISCARDS [54]         zalozil (only when the mover is the player who exchanged)
 *     TAROK_REF_LEGAL    [54]         mozne_vec; 2 bytes of padding follow
 *   meta_out [N,4] i32 (may be NULL): {T, network type (0 Klop, 1 Navadna_igra, 2 Solo, 3 Berac =
 *     Nevronski_igralec.Tipi_NN), rows used (cards played so far), seat to move}.  T is the reference's first
 *     dimension of the two history tensors: the entries of `zgodovina` (cards + the "Talon" entry + Klop's
 *     talon cards: the counter at Igralec.py:456-458 counts them all) rounded up to the next multiple of 8,
 *     plus 8 when already one (:460); T <= 56; the reference's tensors are rows [0, T) of the record's.
 *   Games not in play (finished, waiting for the exchange): an all-zero record and T = 0.
 *   Which tensors a network type consumes (Igralec.py:520-531): Navadna_igra opp, king, own, talon, index,
 *   discards, legal; Solo the same without king; Klop opp, own, talon(54), legal; Berac opp, own, index, legal. */
#define TAROK_REF_ROWS 56
#define TAROK_REF_OPP 0
#define TAROK_REF_OWN 9072
#define TAROK_REF_TALON 12096
#define TAROK_REF_KING 12426
#define TAROK_REF_INDEX 12430
#define TAROK_REF_DISCARDS 12434
#define TAROK_REF_LEGAL 12488
#define TAROK_REF_RECORD_BYTES 12544
int tarok_observe_ref(tarok_env *env, uint8_t *record_out, int32_t *meta_out, void *stream);

/* menjaj_talon_v_vektor (Igralec.py:535-543), the input of the talon-exchange decision, for every game that
 * waits for tarok_exchange: out [N, TAROK_REF_EXCHANGE_BYTES] u8 = roka [54] (the declarer's hand) | talon
 * (54,6) flattened card-major (card c lies in group i: byte 54 + 6c + i) | igra one-hot [15]
 * (igra_zalozi2index, Igralec.py:717-745: (Tri,Dve,Ena) x called suit -> 0..11, Solo_tri/dve/ena -> 12..14)
 * | 7 bytes of padding.  Zero for games in any other phase. */
#define TAROK_REF_EXCHANGE_BYTES 400
int tarok_observe_exchange_ref(tarok_env *env, uint8_t *out, void *stream);

/* The bidding input (pripavi_licitiram, Igralec.py:278-281): out [N,4,54] u8, every seat's hand one-hot. */
int tarok_observe_hands_ref(tarok_env *env, uint8_t *out, void *stream);

/* The play history of a TAROK_HISTORY env, hist [48,N] u8 (device): card p of every slot's current game
 * (entries at or beyond the cards played so far are stale).  tarok_set_state does not touch it: a
 * checkpoint of such an env is the canonical lanes plus this array. */
int tarok_get_history(tarok_env *env, uint8_t *hist_out, void *stream);
int tarok_set_history(tarok_env *env, const uint8_t *hist_in, void *stream);

/* The play mode of an env: HOW the six launches below that turn the network's logits into a card — tarok_sample_policy,
 * tarok_policy_mlp, tarok_policy_step, tarok_policy_step_seats, tarok_policy_step_versus, tarok_policy_step_pool —
 * choose it.  Two numbers,
 * temperature T >= 0 and epsilon in [0, 1]; a new env has (1, 0): one draw from the softmax over the legal cards, as
 * described at those functions.  For a game with k > 0 legal cards, logits l_c and `played` cards so far:
 *   T > 0   the draw is made from p_T(c) ~ exp((l_c - max over the legal cards) * (1.0f / T)): the same spec RNG draw,
 *           192 + played, the same order of additions, the same last-legal-card rule at the top of the CDF;
 *   T = 0   greedy: the lowest-numbered legal card whose logit equals the maximum over the legal cards (p_T is 1 there);
 *           the logits are the float32 values the sampler reads (bf16 widened for tarok_sample_policy);
 *   epsilon with thr = floor(epsilon * 2^24) > 0 a coin is drawn, spec RNG draw 256 + played (the draw indices in use
 *           before end at 255), and iff (coin >> 8) < thr the game plays the Bot's card instead: draw 128 + played, the
 *           card tarok_step_random plays there.  This is Igralec.igraj_karto's arg-max / random_card selection
 *           (Igralec.py:344-355) at T = 0.
 * logp_out is the log of the probability with which the MODE plays the card that was played, explored or not:
 * log((1 - e) p_T(card) + e / k), e = thr / 2^24 — exactly 0 for (0, 0), today's value for (1, 0).  value_out, the
 * features, rows with nothing to play (255, logp 0) and a mixed table's Bot seats (the Bot's card, logp 0) do not depend
 * on the mode; both networks of tarok_policy_step_versus play the env's one mode.
 * The mode is read when a launch is ISSUED: at (1, 0) the launches are the kernels they have always been, otherwise
 * their play-mode twins with the mode's values as kernel arguments.  A graph a caller captured around these launches
 * therefore keeps the mode that was in force at capture, whatever is set later: capture again after a change.
 * tarok_set_play_mode returns TAROK_EINVAL, before any HIP call and leaving the mode as it was, for a NULL env, a NaN,
 * epsilon outside [0, 1], T < 0, 0 < T < 1e-6 or T > 1e6 (1 / T and its products with logit differences stay finite).
 * tarok_get_play_mode returns the two numbers as they were set (either pointer may be NULL). */
int tarok_set_play_mode(tarok_env *env, float temperature, float epsilon);
int tarok_get_play_mode(const tarok_env *env, float *temperature_out, float *epsilon_out);

/* A learned player's igraj_karto (cf. Igralec.py:344-355): sample one LEGAL card per game from
 * policy logits.  logits [N,64] bf16 (card c in column c, columns 54..63 ignored), obs [N] the
 * observation words (legal mask + cards played), softmax over the legal cards only, draw from the
 * spec RNG (draw 192 + cards played).  action_out [N] u8 (255 where nothing is to be played),
 * logp_out [N] f32 log-probability of the drawn card (may be NULL). */
int tarok_sample_policy(tarok_env *env, const void *logits_bf16, const uint64_t *obs,
                        uint8_t *action_out, float *logp_out, void *stream);

/* A whole learned-policy step in one launch: observation features (as tarok_observe) -> MLP
 * 256 -> 256 -> 256 -> 64 with ReLU (bf16 MFMA, f32 accumulate; outputs 0..53 = card logits,
 * output 54 = state value) -> masked categorical sample (as tarok_sample_policy).
 *   w1, w2 (256 outputs), w3 (64 outputs), bf16, 256 inputs each, in MFMA fragment order: the
 *   16-byte element ((o / 32) * 16 + k / 16) * 64 + ((k / 8) % 2) * 32 + o % 32 holds
 *   W[o][8 * (k / 8) .. + 7] of the [out][in] matrix (torch.nn.Linear.weight), i.e.
 *   W.view(out/32, 32, 16, 2, 8).permute(0, 2, 3, 1, 4) — a wave's weight load is then contiguous;
 *   b1, b2 [256] f32, b3 [64] f32;  obs [N] observation words;
 *   action_out [N] u8, logp_out [N] f32 (may be NULL), value_out [N] f32 (may be NULL),
 *   features_out [N,256] bf16 (may be NULL): the features, for the learner's update;
 *   feature_words_out [N,4] u64 (may be NULL): the same 256 features as bits (feature f = bit
 *   f % 64 of word f / 64) — 32 bytes per game instead of 512, for a learner that expands its
 *   minibatches itself. */
int tarok_policy_mlp(tarok_env *env, const void *w1, const float *b1, const void *w2, const float *b2,
                     const void *w3, const float *b3, const uint64_t *obs, uint8_t *action_out,
                     float *logp_out, float *value_out, void *features_out, uint64_t *feature_words_out,
                     void *stream);

/* tarok_policy_mlp followed by tarok_step(action_out, ...) in ONE launch: the workgroup that
 * evaluated the policy for 256 games plays the sampled cards at once (same results as the two
 * calls; saves a launch and its gap per lock-step).  Arguments as in those two functions; obs is
 * the observation BEFORE the step (legal masks), obs_out the one after it (they may not alias). */
int tarok_policy_step(tarok_env *env, const void *w1, const float *b1, const void *w2, const float *b2,
                      const void *w3, const float *b3, const uint64_t *obs, uint8_t *action_out,
                      float *logp_out, float *value_out, uint64_t *feature_words_out, int16_t *reward_out,
                      uint8_t *done_out, uint16_t *trick_out, uint64_t *obs_out, int flags, void *stream);

/* tarok_policy_step with the network on some seats and the Bot (tarok_step_random's card) on the others: the launch
 * of a mixed table, e.g. for playing the same deals with the network on one seat at a time (tarok_amd/evaluate.py).
 *   seats           4-bit set used for every game when seats_per_game is NULL (bit s: seat s plays the network)
 *   seats_per_game  [N] u8 (device) or NULL: the set of each game (bits 4..7 are ignored)
 * The other arguments are tarok_policy_step's.  Rows whose mover is a Bot seat: action_out = the Bot's card,
 * logp_out = 0; value_out and feature_words_out are written for every game.  seats = 15 gives exactly
 * tarok_policy_step; seats = 0 gives the cards, state and outputs of tarok_step_random.  TAROK_EINVAL (before any
 * HIP call) for a NULL env, seats outside 0..15, a missing required array or obs == obs_out. */
int tarok_policy_step_seats(tarok_env *env, int seats, const uint8_t *seats_per_game, const void *w1, const float *b1,
                            const void *w2, const float *b2, const void *w3, const float *b3, const uint64_t *obs,
                            uint8_t *action_out, float *logp_out, float *value_out, uint64_t *feature_words_out,
                            int16_t *reward_out, uint8_t *done_out, uint16_t *trick_out, uint64_t *obs_out, int flags,
                            void *stream);

/* tarok_policy_step_seats with a second network in the Bot's place: two weight sets at one table, e.g. the current
 * checkpoint against an earlier one on the same deals (tarok_amd/evaluate.py, evaluate_vs_policy).
 *   seats, seats_per_game   as in tarok_policy_step_seats: bit s set = seat s plays network A; every other seat
 *                           plays network B
 *   w1 .. b3                network A, v1 .. c3 network B: both in tarok_policy_mlp's layouts
 * The other arguments are tarok_policy_step's.  The mover's network is chosen by the seat field of obs[i] and the
 * game's set, live game or not; action_out, logp_out and value_out of a game are that network's, bit for bit what
 * tarok_policy_mlp with its weights writes on the same observation words (both networks draw with the same spec RNG
 * draw, 192 + cards played, and only one plays: a network's card on a position does not depend on the opponent).
 * action_out = 255 and logp_out = 0 where nothing is to be played; feature_words_out and everything the env half
 * writes are tarok_policy_step's.  seats = 15 gives exactly tarok_policy_step with A, seats = 0 with B.
 * TAROK_EINVAL (before any HIP call) for a NULL env, seats outside 0..15, a missing weight, bias or required array,
 * or obs == obs_out. */
int tarok_policy_step_versus(tarok_env *env, int seats, const uint8_t *seats_per_game, const void *w1, const float *b1,
                             const void *w2, const float *b2, const void *w3, const float *b3, const void *v1,
                             const float *c1, const void *v2, const float *c2, const void *v3, const float *c3,
                             const uint64_t *obs, uint8_t *action_out, float *logp_out, float *value_out,
                             uint64_t *feature_words_out, int16_t *reward_out, uint8_t *done_out, uint16_t *trick_out,
                             uint64_t *obs_out, int flags, void *stream);

/* tarok_policy_step_versus against a POOL of frozen networks in one launch: the seats of a game's set play the learner
 * (w1 .. b3), the others the network of the game's STEP GROUP — group g is slots 256 g .. 256 g + 255, the games one
 * play workgroup owns; a slot stays in its group through auto-resets, so a group keeps its opponent from game to game.
 *   seats, seats_per_game   as in tarok_policy_step_versus: bit s set = seat s plays the learner
 *   pool_size               1 .. TAROK_POOL_MAX networks
 *   p1 .. q3                the pool, six stacked arrays [pool_size, ...]: entry k of an array starts k * size elements
 *                           after its base, size = 65,536 / 256 / 65,536 / 256 / 16,384 / 64 (w1, b1, w2, b2, w3, b3 of
 *                           one network, each entry in tarok_policy_mlp's layout).  Read through the pointers when the
 *                           launch RUNS: a captured graph sees an entry that was overwritten in place
 *   group_net               [ceil(N / 256)] u8 (device) or NULL: the index k of each step group; NULL means
 *                           k = g % pool_size.  ANY k >= pool_size means the learner itself: the group is plain
 *                           self-play (both networks are w1 .. b3), and nothing outside the pool is read
 * The other arguments are tarok_policy_step's.  action_out, logp_out and value_out of a game are its mover's network's,
 * bit for bit what tarok_policy_mlp with that network's weights writes on the same observation words; everything else
 * is tarok_policy_step_versus'.  The env's play mode applies to every network.  seats = 15 gives exactly
 * tarok_policy_step with the learner, whatever the pool; pool_size = 1 with group_net = NULL gives
 * tarok_policy_step_versus(..., pool entry 0) to the byte.
 * TAROK_EINVAL (before any HIP call) for everything tarok_policy_step_versus refuses, pool_size outside
 * 1..TAROK_POOL_MAX or a missing pool array. */
int tarok_policy_step_pool(tarok_env *env, int seats, const uint8_t *seats_per_game, const void *w1, const float *b1,
                           const void *w2, const float *b2, const void *w3, const float *b3, int pool_size,
                           const void *p1, const float *q1, const void *p2, const float *q2, const void *p3,
                           const float *q3, const uint8_t *group_net, const uint64_t *obs, uint8_t *action_out,
                           float *logp_out, float *value_out, uint64_t *feature_words_out, int16_t *reward_out,
                           uint8_t *done_out, uint16_t *trick_out, uint64_t *obs_out, int flags, void *stream);

/* Policy-network playouts: tarok_playout_cards_det whose playouts are played by a policy network — the determinized
 * player with the learned policy inside, a teacher that improves with its student, and (by the choice of net_seats) a
 * best response to a known table.  "Takes part", the worlds and the world key wkey, sum_out [N,12,4] i32, action_out
 * [N] u8, seats / seats_per_game and the read-only contract are exactly tarok_playout_cards_det's.  There is no
 * `samples`: ONE playout per (legal card of rank j, world w < worlds), under the det launch's item key with sample 0,
 *     pkey = game_key(seed ^ salt, gidx, D),   D = 3 << 62 | (u64)ep << 28 | played << 22 | c << 16 | w << 10.
 * Inside a playout, after the candidate card c, the seat to move (absolute seat number) plays
 *   - if its bit is set in net_seats (0..15): the network's GREEDY card — the lowest-numbered legal card at the maximum
 *     of the 54 card logits that tarok_policy_mlp's forward gives (bit for bit) on the feature words of the playout's
 *     own position; the rule of the greedy play mode (tarok_set_play_mode, temperature 0).  The env's own play mode is
 *     not read;
 *   - otherwise the Bot's card, policy_action(pkey, q, legal) at q cards played (spec RNG draw 128 + q), as in
 *     tarok_playout_cards_det.
 * Hence net_seats = 0 writes the bytes of tarok_playout_cards_det(worlds, samples = 1).
 *   w1 .. b3   the network, in tarok_policy_mlp's layouts; read through the pointers when the launch RUNS, so a captured
 *              graph replays with the weights that are in place then
 *   scratch    device memory, 16-byte aligned, at least tarok_playout_net_scratch(env, worlds) bytes (48 bytes per
 *              (game, rank, world)); nothing is allocated inside the call, and the call may be captured into a graph.
 *              Its contents are undefined afterwards.
 * tarok_playout_net_scratch returns TAROK_EINVAL for a NULL env or worlds outside 1..TAROK_PLAYOUT_MAX_WORLDS.
 * TAROK_EINVAL (before any HIP call) for a NULL env, worlds outside 1..TAROK_PLAYOUT_MAX_WORLDS, seats or net_seats
 * outside 0..15, a missing weight or bias, a NULL, misaligned or short scratch, or both outputs NULL. */
int64_t tarok_playout_net_scratch(const tarok_env *env, int worlds);
int tarok_playout_cards_net(tarok_env *env, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game,
                            int net_seats, const void *w1, const float *b1, const void *w2, const float *b2,
                            const void *w3, const float *b3, void *scratch, int64_t scratch_bytes,
                            int32_t *sum_out, uint8_t *action_out, void *stream);

/* tarok_playout_cards_net in the two other fair world kinds: the network plays out worlds the table's knowledge allows.
 * Everything is tarok_playout_cards_net's — "takes part", one playout per (legal card, world) under the same wkey and
 * pkey, net_seats, w1 .. b3 (read when the launches RUN), scratch (tarok_playout_net_scratch(env, worlds) bytes, 16-byte
 * aligned, contents undefined afterwards), sum_out, action_out, three launches on `stream`, nothing allocated, nothing
 * read by the host, the env read-only — except the world that wkey deals:
 *   tarok_playout_cards_net_voids   world w is tarok_playout_cards_voids' under voids[g]: uniform over the re-deals that
 *                                   give no other seat a card of a class its word marks it void in (the fall-backs are
 *                                   that launch's).  voids [N] u32 (device), tarok_shown_voids' words or the caller's
 *                                   own; all-zero words give tarok_playout_cards_net's bytes.
 *   tarok_playout_cards_net_hidden  world w is tarok_playout_cards_hidden's under played[g]: a Klop's face-down talon
 *                                   and, for a mover who is not the declarer, the declarer's discards are re-dealt too.
 *                                   played [N] u64 (device), tarok_played_cards' words.  Where nothing more is hidden the
 *                                   bytes are tarok_playout_cards_net's.
 * The words are an argument: the env needs no history for these calls, and they are read when the launches RUN.  Hence
 * net_seats = 0 writes the bytes of tarok_playout_cards_voids(worlds, 1) / tarok_playout_cards_hidden(worlds, 1).  The
 * two kinds do not compose (as for the Bot-played launches).
 * TAROK_EINVAL (before any HIP call) for everything tarok_playout_cards_net refuses, and for a NULL word array. */
int tarok_playout_cards_net_voids(tarok_env *env, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                  const uint32_t *voids, int net_seats, const void *w1, const float *b1, const void *w2,
                                  const float *b2, const void *w3, const float *b3, void *scratch, int64_t scratch_bytes,
                                  int32_t *sum_out, uint8_t *action_out, void *stream);
int tarok_playout_cards_net_hidden(tarok_env *env, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                   const uint64_t *played, int net_seats, const void *w1, const float *b1, const void *w2,
                                   const float *b2, const void *w3, const float *b3, void *scratch, int64_t scratch_bytes,
                                   int32_t *sum_out, uint8_t *action_out, void *stream);

/* Value-bootstrapped net playouts: the three launches above with every playout stopped at the VIEWER's depth-th next
 * decision, where the network's value head stands in for the rest of the game.  "Takes part", the worlds, wkey and pkey,
 * the item numbering, net_seats, w1 .. b3 (read when the launches RUN), the scratch and its size
 * (tarok_playout_net_scratch(env, worlds), 16-byte aligned, contents undefined afterwards), sum_out, action_out, the
 * read-only env, three launches on `stream`, nothing allocated and nothing read by the host are the existing kind's:
 *   kind = TAROK_NET_WORLDS_DET     tarok_playout_cards_net's worlds;         words = NULL
 *   kind = TAROK_NET_WORLDS_VOIDS   tarok_playout_cards_net_voids' worlds;    words = voids  [N] u32 (device)
 *   kind = TAROK_NET_WORLDS_HIDDEN  tarok_playout_cards_net_hidden's worlds;  words = played [N] u64 (device)
 * What is new:
 *   - the VIEWER of an item is the seat to move in the env's position (the seat that plays the candidate card, the
 *     seat the playouts are for);
 *   - after the candidate, a live item counts the positions at which the viewer is to move.  At the depth-th such
 *     position the item STOPS without playing a card.  (A seat plays once per trick: at depth = 1 an item plays at
 *     most 6 cards after the candidate and stops in its 7th card round at the latest.)
 *   - at the stop, tarok_policy_mlp's forward runs on that position's feature words with w1 .. b3, whether or not the
 *     viewer is in net_seats; v is its output 54, bit for bit what tarok_policy_mlp writes to value_out there.  The
 *     position is the viewer's own decision, so v depends on the world only through the cards played in it: own hand,
 *     legal cards, table, taken cards, contract and team are what the viewer knows;
 *   - the number written is computed in float32:  t = v * value_scale;  t = 0 if t is NaN;  t clamped to
 *     [-32767, 32767];  V = (int)rintf(t), ties to even.  (value_scale = 1 / reward_scale turns a value head trained on
 *     returns in reward_scale points back into points.)
 *   - the stopped item's result is V in the viewer's column and 0 in the other three; an item whose game ends before
 *     the stop keeps its four true scores, as in the existing launches.
 * ONLY THE VIEWER'S COLUMN of sum_out is meaningful where items stopped: the other three columns sum true scores of the
 * finished items and zeros of the stopped ones.  action_out keeps the card rule of the existing launches, which reads
 * the mover's (= the viewer's) column alone.
 * After its candidate the viewer has at most 11 decisions left, so depth = TAROK_PLAYOUT_MAX_DEPTH = 12 never stops an
 * item and writes the bytes of the existing launch of the kind, for any weights and any value_scale.
 * TAROK_EINVAL (before any HIP call) for everything the existing launch of the kind refuses, kind outside 0..2, words
 * NULL for kind 1 or 2 or non-NULL for kind 0, depth outside 1..TAROK_PLAYOUT_MAX_DEPTH, value_scale not finite or
 * not > 0. */
#define TAROK_NET_WORLDS_DET 0
#define TAROK_NET_WORLDS_VOIDS 1
#define TAROK_NET_WORLDS_HIDDEN 2
#define TAROK_PLAYOUT_MAX_DEPTH 12
int tarok_playout_cards_net_value(tarok_env *env, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                  int kind, const void *words, int net_seats, int depth, float value_scale,
                                  const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                                  const float *b3, void *scratch, int64_t scratch_bytes, int32_t *sum_out,
                                  uint8_t *action_out, void *stream);

/* Sequential-halving playouts: tarok_playout_cards_det / _voids / _hidden whose later worlds are played only by the
 * leading cards.  One launch; exact and integer.  kind: TAROK_NET_WORLDS_DET / _VOIDS / _HIDDEN (the name is historical:
 * here it names the Bot-played launch whose worlds are dealt); words: NULL, the voids [N] u32 or the played [N] u64, exactly
 * as tarok_playout_cards_net_value takes them.  rounds: 1..TAROK_PLAYOUT_MAX_ROUNDS; round_worlds: a HOST array of
 * `rounds` positive ints, read during the call; W = their sum <= TAROK_PLAYOUT_MAX_WORLDS; samples as in those launches.
 *
 * "Takes part", the position, wkey, pkey, ebase, the rank j of a legal card and the Bot's card for a mover outside the
 * seat set are the existing card launches', word for word.  World w, w < W, is the world the existing launch of that kind
 * deals under w.  With e_r the cumulative sum of round_worlds (e_{-1} = 0), round r covers the worlds e_{r-1} .. e_r - 1:
 * every card ALIVE in round r is played `samples` times in each of them under the existing item key
 * (c << 16 | w << 10 | k) and the four scores are added to the card's row.
 *   Before round 0 every legal rank is alive.
 *   After a round that is not the last, with k cards alive, the max(1, ceil(k / 2)) cards with the highest mover's sum
 *   stay alive, ties to the lower rank.  (All alive cards have had the same number of playouts: comparing sums is
 *   comparing means.)
 *   A game with one card alive plays no further round.
 *   sum_out    [N,12,4] i32, 16-byte aligned, or NULL: row j = the four scores summed over the playouts card j got; zero
 *              rows beyond the legal cards and for games that do not take part.
 *   count_out  [N,12] i32, 16-byte aligned, or NULL: entry j = the playouts behind row j, (worlds played) x samples; 0
 *              beyond the legal cards and for games that do not take part.
 *   action_out [N] u8 or NULL: among the cards alive after the last round played, the lowest rank at the maximum of the
 *              mover's sum; the Bot's card or 255 under the existing rule.
 * EVERY row of every given output is written.  Read-only on the env, stream-ordered, capturable: the rounds cost no
 * launches, no global traffic and no host read.
 * Consequences: rounds = 1 writes the bytes of tarok_playout_cards_det / _voids / _hidden(W, samples), and count =
 * W * samples on the legal ranks; for any schedule a row whose count is e * samples equals that rank's row of the
 * existing launch at worlds = e, e one of the cumulative ends (the keys depend on no launch size).
 * TAROK_EINVAL (before any HIP call) for everything the existing launch of that kind refuses, rounds outside
 * 1..TAROK_PLAYOUT_MAX_ROUNDS, a NULL round_worlds, an entry < 1, W > TAROK_PLAYOUT_MAX_WORLDS, a kind outside the three,
 * words NULL for a kind that needs them or non-NULL for kind 0, all three outputs NULL. */
#define TAROK_PLAYOUT_MAX_ROUNDS 4
int tarok_playout_cards_halving(tarok_env *env, int kind, const void *words, int rounds, const int *round_worlds, int samples,
                                uint64_t salt, int seats, const uint8_t *seats_per_game, int32_t *sum_out, int32_t *count_out,
                                uint8_t *action_out, void *stream);

/* tarok_playout_targets for sums with a count per card (a halving launch's sum_out and count_out).  The "has a teacher"
 * rule and the row layout are tarok_playout_targets'.  With a teacher, nl as there:
 *   m_j = float(sums[g][j][s]) / float(counts[g][j]), one float32 division, for the ranks j < nl with counts[g][j] > 0;
 *   z_j = (m_j - max_k m_k) / tau over those ranks; target = bf16(exp(z_j) / sum_k exp(z_k)) at the rank's card.
 *   A legal rank with count <= 0 gets target 0; a game all of whose legal ranks have count <= 0 gets a zero row.  (Neither
 *   happens on a halving launch's own output, but the call is a function of its arguments.)
 *   tau = 0: 1.0 at the lowest rank at the maximum of m AMONG THE RANKS OF MAXIMAL COUNT, compared exactly (equal counts:
 *   the integer sums).  On a halving launch's output this is the launch's action_out.
 * sums [N,12,4] i32 and counts [N,12] i32, both 16-byte aligned; obs, seats, seats_per_game, target_out as there.
 * TAROK_EINVAL (before any HIP call) for a NULL env or array (seats_per_game may be NULL), tau < 0, NaN or infinite, a
 * tau > 0 that is not a normal float32 number (below 2^-126), seats outside 0..15. */
int tarok_playout_targets_counts(tarok_env *env, const int32_t *sums, const int32_t *counts, const uint64_t *obs, float tau,
                                 int seats, const uint8_t *seats_per_game, void *target_out, void *stream);

/* Sequential-halving NET playouts on a compacted item list: tarok_playout_cards_halving's definition at samples = 1, its
 * playouts played as tarok_playout_cards_net / _voids / _hidden / _value play theirs.  kind, words, rounds
 * and round_worlds as tarok_playout_cards_halving takes them; salt, seats, seats_per_game, net_seats and w1 .. b3 (read
 * when the launches RUN) as tarok_playout_cards_net.  World w and the item key (c << 16 | w << 10) are the existing net
 * launch's; neither depends on a launch size.  With e0 / e1 the cumulative world counts before / after round r, the round
 * plays every rank still alive once in each of the worlds e0 .. e1 - 1; after a round that is not the last the better half
 * by the mover's column stays (the rule above); a game down to one alive card plays no further round.
 *   depth      0 or TAROK_PLAYOUT_MAX_DEPTH: every playout runs to the last card.  1 .. TAROK_PLAYOUT_MAX_DEPTH - 1: it
 *              stops at the viewer's depth-th decision with value_scale x the value head in the viewer's column, as
 *              tarok_playout_cards_net_value stops it; only that column is meaningful, and the rule reads no other.
 *   value_scale finite and > 0 (read only where depth stops a playout).
 *   sum_out    [N,12,4] i32, count_out [N,12] i32 (both 16-byte aligned), action_out [N] u8: each optional, at least one
 *              given.  count_out[g][j] is the cumulative end e1 of the last round rank j played (0: none); the card is
 *              the lowest rank at the maximum of the mover's sum among the ranks alive at the end, the Bot's card for a
 *              game in play that does not take part, 255 elsewhere.
 * Consequences: rounds = 1, (W), writes the sum_out and action_out of the existing net launch of that kind and depth at
 * worlds = W, byte for byte; a row whose count is e equals the existing launch's row at worlds = e.  net_seats = 0 writes
 * tarok_playout_cards_halving(kind, schedule, samples = 1)'s three outputs.
 *
 * The launches (all on `stream`; no host read, no allocation, no synchronisation: capturable).  One init launch, then per
 * round: three launches of an exclusive prefix sum over the games' item counts popc(on[g]) x W_r (on[g]: the ranks of
 * game g that play the round), which give every game its first slot and the round's total in a device word; the items, in
 * ascending (game, rank, world) order — the item of the q-th set bit of on[g] in world w is base[g] + q x W_r + (w - e0) —;
 * the playouts, over a grid sized by the round's BOUND n x a_r x W_r (a_0 = 12, a_{r+1} = ceil(a_r / 2): 12, 6, 3, 2),
 * whose workgroups past the total run nothing; the sums and the survivor rule.
 *
 * scratch: device memory, 16-byte aligned, contents undefined afterwards.  tarok_playout_net_halving_scratch_bytes:
 *     B = max over the rounds of n x a_r x W_r                                (the largest round's item bound)
 *     bytes = 48 x B + 252 x n + 4 x ceil(n / 256) + 4, rounded up to a multiple of 16
 * — the four item arrays at B (48 bytes an item), per game the running [12][4] sums (192), [12] counts (48) and the words
 * on, alive and base (12), the scan's partials (a word per 256 games) and the total word.
 * tarok_playout_net_halving_scratch_bytes returns TAROK_EINVAL for a NULL env, rounds outside 1..TAROK_PLAYOUT_MAX_ROUNDS, a
 * NULL round_worlds, an entry < 1, a sum above TAROK_PLAYOUT_MAX_WORLDS or a round whose bound reaches 2^31 items.
 * TAROK_EINVAL (before any HIP call) for all of those, a kind outside the three, words NULL for a kind that needs them or
 * non-NULL for kind 0, seats or net_seats outside 0..15, a NULL weight array, depth outside 0..TAROK_PLAYOUT_MAX_DEPTH,
 * value_scale not finite or <= 0, a NULL or misaligned scratch or scratch_bytes below the size, all three outputs NULL. */
int64_t tarok_playout_net_halving_scratch_bytes(const tarok_env *env, int rounds, const int *round_worlds);
int tarok_playout_cards_net_halving(tarok_env *env, int kind, const void *words, int rounds, const int *round_worlds,
                                    uint64_t salt, int seats, const uint8_t *seats_per_game, int net_seats, const void *w1,
                                    const float *b1, const void *w2, const float *b2, const void *w3, const float *b3, int depth,
                                    float value_scale, void *scratch, int64_t scratch_bytes, int32_t *sum_out,
                                    int32_t *count_out, uint8_t *action_out, void *stream);

/* Two-network net playouts with VIEWER-RELATIVE seats: tarok_playout_cards_net_value and
 * tarok_playout_cards_net_halving whose playouts seat two networks, A (w1 .. b3) and B (v1 .. c3, in the same layouts), by
 * where a seat sits relative to the item's viewer.  The VIEWER of an item is the seat to move in the env's position (the
 * seat that plays the candidate card, the seat the playouts are for), as in tarok_playout_cards_net_value.  For an item
 * whose viewer is v, the RELATIVE seat of absolute seat s is r = (s - v) & 3: r = 0 is the viewer, r = 1 the seat after
 * it.  Two 4-bit sets over r give the roles:
 *   own_rel   the relative seats that play network A;
 *   opp_rel   the relative seats that play network B.
 * Inside a playout, after the candidate card, the seat to move at relative seat r plays
 *   - r in own_rel: A's GREEDY card — the lowest-numbered legal card at the maximum of the 54 card logits that
 *     tarok_policy_mlp's forward gives (bit for bit) with A on the feature words of the playout's own position;
 *   - r in opp_rel: B's greedy card, by the same rule with B;
 *   - r in neither: the Bot's card policy_action(pkey, q, legal) at q cards played, as in tarok_playout_cards_det.
 * own_rel & opp_rel != 0 is TAROK_EINVAL.  own_rel = 1, opp_rel = 14: A plays the viewer, B plays the table — the playouts
 * of a best response to B, and of an opponent model.  One launch serves every game's own viewer.
 * With depth > 0 an item stops at the viewer's depth-th decision exactly as in tarok_playout_cards_net_value; the value v is
 * output 54 of the VIEWER'S OWN network on the stop position — B if bit 0 of opp_rel is set, else A, whether or not the
 * viewer is in either set — and t = v * value_scale, NaN -> 0, the clamp to [-32767, 32767], V = (int)rintf(t) and "V in the
 * viewer's column, 0 in the other three" are that launch's.  depth = 0 and depth = TAROK_PLAYOUT_MAX_DEPTH play to the last
 * card; value_scale is then not read by the launches (it is still checked).
 * Everything else is the existing launches': kind and words as tarok_playout_cards_net_value takes them; "takes part", the
 * worlds and wkey, pkey, the item numbering, seats / seats_per_game, sum_out [N,12,4] i32, action_out [N] u8, count_out
 * [N,12] i32, rounds and round_worlds, the survivor rule, the prefix-sum launches, the read-only env; the scratch sizes are
 * tarok_playout_net_scratch(env, worlds) and tarok_playout_net_halving_scratch_bytes(env, rounds, round_worlds).  BOTH weight
 * sets are read through the pointers when the launches RUN: a captured graph replays with whatever A and B hold then.
 * Nothing is allocated, nothing is read by the host; three launches (the items, whose markers carry the viewer at every
 * depth; the playouts; the sums), or the halving launch's per round.
 * Consequences, byte for byte: (own_rel, opp_rel) = (15, 0) with any B (or none) is net_seats = 15 on A; (0, 15) is
 * net_seats = 15 on B; any split of the four seats between equal A and B is net_seats = 15; (0, 0) is
 * tarok_playout_cards_det / _voids / _hidden(worlds, 1); at seats = 1 << v, own_rel = an absolute set m rotated right by v
 * (bit r of own_rel = bit (r + v) & 3 of m) with opp_rel = 0 is net_seats = m.
 * B may be NULL (all six) when opp_rel = 0: it is not read.  The exchange and bid launches have no versus form.
 * TAROK_EINVAL (before any HIP call) for everything tarok_playout_cards_net_value / tarok_playout_cards_net_halving refuse
 * (net_seats aside: there is none), depth outside 0..TAROK_PLAYOUT_MAX_DEPTH, value_scale not finite or not > 0, own_rel or
 * opp_rel outside 0..15, own_rel & opp_rel != 0, a missing array of B when opp_rel != 0. */
int tarok_playout_cards_net_versus(tarok_env *env, int worlds, uint64_t salt, int seats, const uint8_t *seats_per_game,
                                   int kind, const void *words, int own_rel, int opp_rel, int depth, float value_scale,
                                   const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                                   const float *b3, const void *v1, const float *c1, const void *v2, const float *c2,
                                   const void *v3, const float *c3, void *scratch, int64_t scratch_bytes, int32_t *sum_out,
                                   uint8_t *action_out, void *stream);
int tarok_playout_cards_net_versus_halving(tarok_env *env, int kind, const void *words, int rounds, const int *round_worlds,
                                           uint64_t salt, int seats, const uint8_t *seats_per_game, int own_rel, int opp_rel,
                                           const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                                           const float *b3, const void *v1, const float *c1, const void *v2, const float *c2,
                                           const void *v3, const float *c3, int depth, float value_scale, void *scratch,
                                           int64_t scratch_bytes, int32_t *sum_out, int32_t *count_out, uint8_t *action_out,
                                           void *stream);

/* SAMPLED net playouts: tarok_playout_cards_net_versus (dense; the three world kinds; viewer-relative roles;
 * the optional value stop) whose networks play as they play AT THE TABLE — each under a play mode of its own — and with
 * `samples` playouts per (legal card, world).
 * ITEMS.  One item per (game g, rank j, world w, sample k), samples in 1..TAROK_PLAYOUT_MAX_SAMPLES, numbered
 *   item = ((g * 12 + j) * worlds + w) * samples + k.
 * All samples of a world start from the same dealt position (the world is dealt once, under the launches' wkey).  Item k's key
 * is the item key of the net launches with k in its ten low bits, which every other net item kernel leaves 0:
 *   ikey = game_key(seed ^ salt, offset + g, 3 << 62 | episode << 28 | played << 22 | card << 16 | w << 10 | k),
 * the pkey of tarok_playout_cards_det / _voids / _hidden(worlds, samples).
 * PLAY MODES.  (temperature_a, epsilon_a) is network A's and (temperature_b, epsilon_b) network B's: the two arguments of
 * tarok_set_play_mode, taken with its validation and its conversion (inv_t = 1 / temperature, greedy at temperature 0,
 * thr = floor(epsilon * 2^24), eps = thr / 2^24).  Inside a playout, after the candidate card, the seat to move at q cards
 * played, at relative seat r, plays
 *   - r in own_rel: what the table's sampler gives on tarok_policy_mlp's 54 card logits of A (bit for bit) on the playout's
 *     own position, with key = ikey, played = q and A's mode: the tempered inverse-CDF draw on spec RNG draw 192 + q (the
 *     lowest-numbered legal card at the maximum at temperature 0) — unless A's coin, draw 256 + q, says explore
 *     ((coin >> 8) < thr): then the Bot's card policy_action(ikey, q, legal);
 *   - r in opp_rel: the same with B and B's mode;
 *   - r in neither: the Bot's card policy_action(ikey, q, legal), as before.
 * The three draws of a position use counters 128 + q, 192 + q and 256 + q of one key: they are independent.
 * The value stop (depth > 0) reads output 54 of the viewer's own network exactly as tarok_playout_cards_net_versus does; no
 * mode touches it.  The env's own play mode is neither read nor written.
 * OUTPUTS.  sum_out [N,12,4] i32 is the sum over the worlds x samples items of a row; action_out [N] u8 follows
 * card_epilogue's rule on it, as in every card launch.  Scratch: 48 bytes per item,
 * tarok_playout_cards_net_sampled_scratch(env, worlds, samples); TAROK_EINVAL where worlds or samples are out of range or
 * the count reaches 2^31 items.  Three launches (items, playouts, sums) on `stream`; nothing is allocated, nothing read by the
 * host; both weight sets are read when the launches RUN.
 * Consequences, byte for byte: samples = 1 with both temperatures 0 and both epsilons 0 is tarok_playout_cards_net_versus;
 * (own_rel, opp_rel) = (0, 0) at any modes, and epsilon 1 on both networks at any roles, is tarok_playout_cards_det / _voids /
 * _hidden(worlds, samples) (where nothing stops, depth 0 or 12; with a stop, the (0, 0) rows of the same depth); (15, 0) at temperature 0 and epsilon 0 with S samples gives S x the samples = 1 rows; equal A
 * and B under equal modes give (15, 0)'s rows for any split of the four seats.
 * TAROK_EINVAL (before any HIP call) for everything tarok_playout_cards_net_versus refuses, samples outside
 * 1..TAROK_PLAYOUT_MAX_SAMPLES, an item count of 2^31 or more, and a temperature or epsilon tarok_set_play_mode refuses (NaN,
 * epsilon outside [0, 1], temperature < 0, in (0, 1e-6) or > 1e6) — B's mode is checked also where opp_rel = 0. */
int64_t tarok_playout_cards_net_sampled_scratch(const tarok_env *env, int worlds, int samples);
int tarok_playout_cards_net_sampled(tarok_env *env, int worlds, int samples, uint64_t salt, int seats,
                                    const uint8_t *seats_per_game, int kind, const void *words, int own_rel, int opp_rel,
                                    int depth, float value_scale, float temperature_a, float epsilon_a, float temperature_b,
                                    float epsilon_b, const void *w1, const float *b1, const void *w2, const float *b2,
                                    const void *w3, const float *b3, const void *v1, const float *c1, const void *v2,
                                    const float *c2, const void *v3, const float *c3, void *scratch, int64_t scratch_bytes,
                                    int32_t *sum_out, uint8_t *action_out, void *stream);

/* Net-played playouts for the exchange and the bid: tarok_playout_exchange and tarok_playout_bids at ONE playout per
 * (candidate or option, world), played as tarok_playout_cards_net plays its playouts — the network's greedy card on the
 * absolute seats of net_seats (one launch-wide 4-bit set), the Bot's card policy_action(pkey, q, legal) on the others.
 * There is no `samples`: the playout of a row in world w runs under the Bot launch's pkey with k = 0.  Hence
 * net_seats = 0 writes the bytes of tarok_playout_exchange(worlds, 1, discard_sets) and of tarok_playout_bids(worlds, 1).
 * w1 .. b3, scratch (16-byte aligned, contents undefined afterwards), the read-only contract and the capture rule are
 * tarok_playout_cards_net's: nothing is allocated inside either call, the weights are read when the launches RUN.
 *
 * tarok_playout_exchange_net: "waiting" and "takes part", the worlds (wkey), the candidates (ckey), sum_out
 *   [N, 6 * discard_sets, 4] i32 (16-byte aligned), choice_out [N] i8 and discards_out [N,3] u8 — each or NULL, EVERY row
 *   written, the Bot's own exchange for a waiting game outside the seat set, -1 / 255 for a game that does not wait —
 *   are exactly tarok_playout_exchange's; the sums are over `worlds` playouts.  Three launches.  Scratch: 48 bytes per
 *   item, item (g * 6 * discard_sets + r) * worlds + w.
 * tarok_playout_bids_net: the deal (episode, deals), the viewers, the worlds (wkey), the rows of `contracts`, the Bot's
 *   exchange under pkey and sum_out [N,4,TAROK_BID_ROWS] i32 — the viewer's own score; zeros for seats outside the set,
 *   rows outside `contracts`, an invalid deal row and row 19: the pass is not valued here — are exactly
 *   tarok_playout_bids'.  Four launches (the deal first).  Scratch: 48 bytes per item, item ((g * 4 + v) * TAROK_BID_ROWS
 *   + r) * worlds + w, then the deal's 40 bytes per game: unlike tarok_playout_bids the first call allocates nothing.
 * The _scratch functions return TAROK_EINVAL for a NULL env or a size argument out of range.
 * TAROK_EINVAL (before any HIP call) for a NULL env, worlds outside 1..TAROK_PLAYOUT_MAX_WORLDS, discard_sets outside
 * 1..TAROK_EXCHANGE_MAX_SETS, contracts outside 1..TAROK_BID_ALL_CONTRACTS, seats or net_seats outside 0..15, a missing
 * weight or bias, a NULL, misaligned or short scratch, or every output NULL. */
int64_t tarok_playout_exchange_net_scratch(const tarok_env *env, int worlds, int discard_sets);
int tarok_playout_exchange_net(tarok_env *env, int worlds, int discard_sets, uint64_t salt, int seats,
                               const uint8_t *seats_per_game, int net_seats, const void *w1, const float *b1, const void *w2,
                               const float *b2, const void *w3, const float *b3, void *scratch, int64_t scratch_bytes,
                               int32_t *sum_out, int8_t *choice_out, uint8_t *discards_out, void *stream);
int64_t tarok_playout_bids_net_scratch(const tarok_env *env, int worlds);
int tarok_playout_bids_net(tarok_env *env, uint32_t episode, const uint8_t *deals, int worlds, int contracts, uint64_t salt,
                           int seats, const uint8_t *seats_per_game, int net_seats, const void *w1, const float *b1,
                           const void *w2, const float *b2, const void *w3, const float *b3, void *scratch,
                           int64_t scratch_bytes, int32_t *sum_out, void *stream);

/* Value-stopped net playouts for the exchange, the bid and the pass: the two launches above with every playout stopped
 * at the VIEWER's depth-th decision, as tarok_playout_cards_net_value stops a card's playouts.  The worlds, candidates,
 * rows, keys (k = 0), item numbering, the Bot's exchange inside a bid item, net_seats, "takes part", the outputs' shapes
 * and rules, the scratch and its size (tarok_playout_exchange_net_scratch / tarok_playout_bids_net_scratch), the read-only
 * env, three / four launches on `stream`, nothing allocated are the existing launches', word for word.  The stop, the
 * forward at the stop, the float32 steps to V = rint(clamp(v54 * value_scale)) and the stopped item's result (V in the
 * viewer's column, 0 in the other three; an item whose game ends first keeps its four true scores) are
 * tarok_playout_cards_net_value's.  What is new:
 *   - the VIEWER of an exchange item is the declarer; of a bid item, the seat v whose row it is — in the Klop row too,
 *     where seat 0 declares, and in a pass item, where another seat declares.  choice_out / discards_out read the
 *     declarer's column of the sums and sum_out of the bids holds the viewer's: both are the column V lands in;
 *   - DEPTH RANGE 1..TAROK_PLAYOUT_FRONT_MAX_DEPTH = 13, not 12: an item starts at 0 cards played, so its viewer has all
 *     12 decisions ahead (after a candidate card it has 11).  Depth 13 never stops an item and writes the bytes of the
 *     existing launch for any weights and value_scale; depth 12 stops every item at the viewer's forced last card.  This
 *     is the one place where the launches differ from tarok_playout_cards_net_value;
 *   - pass_value = 1 (bids): slot (g, v, 19, w) is a live item for every viewer of the seat set — tarok_playout_bids_pass'
 *     item under that launch's pkey with r = 19 and k = 0: three Bots bid with v muted, their contract, declarer and king
 *     are set up on v's world, the Bot exchanges where the game has an exchange, and the item is played and stopped as a
 *     row's item is.  sum_out[g][v][19] is then v's value of a pass; with depth 13 and net_seats = 0 the twenty rows are
 *     tarok_playout_bids_pass(worlds, 1)'s bytes.  pass_value = 0: row 19 stays 0.
 * At depth 1 with the viewer on lead the stop is at 0 cards played: no card is played, and V depends on the world only
 * through what the viewer knows, so a candidate's (an option's) number is the same in every world.  That is correct and
 * cheap; extra worlds add nothing there.
 * TAROK_EINVAL (before any HIP call) for everything the existing launch refuses, depth outside
 * 1..TAROK_PLAYOUT_FRONT_MAX_DEPTH, value_scale not finite or not > 0, pass_value outside 0..1. */
#define TAROK_PLAYOUT_FRONT_MAX_DEPTH 13
int tarok_playout_exchange_net_value(tarok_env *env, int worlds, int discard_sets, uint64_t salt, int seats,
                                     const uint8_t *seats_per_game, int net_seats, int depth, float value_scale,
                                     const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                                     const float *b3, void *scratch, int64_t scratch_bytes, int32_t *sum_out,
                                     int8_t *choice_out, uint8_t *discards_out, void *stream);
int tarok_playout_bids_net_value(tarok_env *env, uint32_t episode, const uint8_t *deals, int worlds, int contracts,
                                 uint64_t salt, int seats, const uint8_t *seats_per_game, int net_seats, int depth,
                                 float value_scale, int pass_value, const void *w1, const float *b1, const void *w2,
                                 const float *b2, const void *w3, const float *b3, void *scratch, int64_t scratch_bytes,
                                 int32_t *sum_out, void *stream);

/* The four launches above on a COMPACTED item list: the existing launches' definition, word for word —
 * "waiting", "takes part", worlds, candidates, rows, keys (k = 0), the Bot's exchange inside a bid item and a pass item, the
 * viewer, every output's shape, and the rule that every row is written — with the items laid without gaps, so a play tile's
 * 128 forward rows are live items only.
 *   depth      0 or TAROK_PLAYOUT_FRONT_MAX_DEPTH: every item is played to the last card.  1..12: an item stops at the
 *              viewer's depth-th decision exactly as the _value launches stop it.
 *   value_scale finite and > 0; read only where depth stops an item.
 *   pass_value (bids) 0 or 1, at any depth; at depth 0 or 13 it is tarok_playout_bids_net_value(depth = 13, pass_value = 1).
 * Consequences, for any weights: at depth 0 or 13 with pass_value = 0 the outputs are the bytes of tarok_playout_exchange_net /
 * tarok_playout_bids_net; at every other (depth, pass_value) those of tarok_playout_exchange_net_value /
 * tarok_playout_bids_net_value; hence net_seats = 0 gives tarok_playout_exchange(worlds, 1, sets) and
 * tarok_playout_bids(worlds, 1) / tarok_playout_bids_pass(worlds, 1).
 *
 * The list.  A UNIT is one (game, talon group) for the exchange — 6 n units, unit g * 6 + i, whose live rows are the set
 * indices d < discard_sets of a group the contract has in a game that takes part — and one (game, viewer) for the bids —
 * 4 n units, unit g * 4 + v, whose live rows are the rows of `contracts`, plus row 19 with pass_value, for a viewer of the
 * seat set with a valid deal row.  Each unit has a u32 `on` word of its live rows; the item of the q-th set bit in world w
 * is base[u] + q x worlds + w, base the exclusive prefix sum of popc(on) x worlds over the units: the items ascend in
 * (game, group or viewer, row, world).
 *
 * The launches (all on `stream`; no host read, no allocation, no synchronisation: capturable, the bids' first call
 * included): for the bids the deal; the on words; the three launches of tarok_playout_cards_net_halving's prefix sum, over
 * the units; the items, every slot below the list's total and none at or above it; the playouts, over a grid sized by the
 * host's BOUND, whose workgroups past the total run nothing; the sums (and the exchange's choice).
 *
 * The bound B, which the host computes without reading the env:
 *     exchange  B = n x 6 x discard_sets x worlds — every slot of the dense grid: the item arrays do NOT shrink (that would
 *               need the contracts on the host); the gain is the playouts' time;
 *     bids      B = n x U x R x worlds, U = popc(seats) without seats_per_game, else 4; R = the rows of `contracts` (1 for
 *               Klop, 4 each for Tri / Dve / Ena, 1 for each contract above) + pass_value.
 * scratch: device memory, 16-byte aligned, contents undefined afterwards.  With units = 6 n / 4 n:
 *     bytes = 48 x B + [bids: 40 x n] + 8 x units + 4 x ceil(units / 256) + 4, rounded up to a multiple of 16
 * — the four item arrays at B, the bids' deal, the units' on and base words, the scan's partials and the total word, in
 * that order.  tarok_playout_bids_net_list_scratch takes the seat set the launch will get and per_game_seats = 1 where it
 * will get a seats_per_game array.
 * The _scratch entries return TAROK_EINVAL for a NULL env, worlds outside 1..TAROK_PLAYOUT_MAX_WORLDS, discard_sets outside
 * 1..TAROK_EXCHANGE_MAX_SETS, contracts outside 1..TAROK_BID_ALL_CONTRACTS, seats outside 0..15, per_game_seats or pass_value
 * outside 0..1, and a bound that reaches 2^31 items.  The launches: TAROK_EINVAL (before any HIP call) for all of those, for
 * everything the existing launches refuse, depth outside 0..TAROK_PLAYOUT_FRONT_MAX_DEPTH, value_scale not finite or <= 0, a
 * NULL or misaligned scratch or scratch_bytes below the size. */
int64_t tarok_playout_exchange_net_list_scratch(const tarok_env *env, int worlds, int discard_sets);
int tarok_playout_exchange_net_list(tarok_env *env, int worlds, int discard_sets, uint64_t salt, int seats,
                                    const uint8_t *seats_per_game, int net_seats, int depth, float value_scale,
                                    const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                                    const float *b3, void *scratch, int64_t scratch_bytes, int32_t *sum_out,
                                    int8_t *choice_out, uint8_t *discards_out, void *stream);
int64_t tarok_playout_bids_net_list_scratch(const tarok_env *env, int worlds, int contracts, int seats, int per_game_seats,
                                            int pass_value);
int tarok_playout_bids_net_list(tarok_env *env, uint32_t episode, const uint8_t *deals, int worlds, int contracts,
                                uint64_t salt, int seats, const uint8_t *seats_per_game, int net_seats, int depth,
                                float value_scale, int pass_value, const void *w1, const float *b1, const void *w2,
                                const float *b2, const void *w3, const float *b3, void *scratch, int64_t scratch_bytes,
                                int32_t *sum_out, void *stream);

/* The two list launches above with SEQUENTIAL HALVING: later worlds are spent only on the leading candidates
 * of a game, or the leading rows of a (game, viewer).  The arguments are the _net_list launches', with `rounds,
 * round_worlds` in the place of `worlds`: round_worlds is a HOST array of `rounds` ints, read during the call, under
 * tarok_playout_cards_net_halving's rules — rounds 1..TAROK_PLAYOUT_MAX_ROUNDS, every entry >= 1, W = their sum <=
 * TAROK_PLAYOUT_MAX_WORLDS.  depth 0 or TAROK_PLAYOUT_FRONT_MAX_DEPTH: every item is played to the last card; 1..12: an
 * item stops at the viewer's depth-th decision, as in the list launches.  value_scale finite and > 0.  pass_value (bids) 0
 * or 1 at any depth.
 *
 * The existing launches' definition stays word for word: "waiting" and "takes part", the worlds (wkey), the candidates
 * (ckey) and the rows, the playout keys with k = 0, the Bot's exchange inside a bid item and a pass item, the viewer, and
 * net_seats.  No key depends on a launch size: world w is the world every existing launch deals under w.
 *
 * The rounds.  With e0 / e1 the cumulative world counts before / after round r, round r plays every ARM still alive once in
 * each of the worlds e0 .. e1 - 1.
 *   exchange   the arms of a game that takes part are its candidates r = i x D + d (i < its groups, d < D = discard_sets),
 *              compared by the declarer's column of the running sums;
 *   bids       the arms of a unit (g, v) are the rows of `contracts`, compared by the viewer's running sum;
 *   the pass   with pass_value = 1 row 19 is NOT an arm: it is the bar every answer is held to, played in every round its
 *              unit plays and never eliminated.
 * The survivor rule, after a round that is not the last, with k arms alive and keep = max(1, ceil(k / 2)): arm j stays iff
 * fewer than `keep` alive arms beat it, arm a beating j when S_a > S_j, or S_a = S_j and a < j (the highest sums stay, ties to
 * the lower index: tarok_playout_cards_halving's rule).  A game or unit with one arm alive plays no further round, and
 * neither does its pass item.
 *
 * Outputs: each optional, at least one given; EVERY row is written.
 *   exchange   sum_out [N, 6 D, 4] i32 the running sums; count_out [N, 6 D] i32 the cumulative end e1 of the last round the
 *              candidate played (0: none); choice_out [N] i8 / discards_out [N,3] u8: for a game that takes part the first
 *              candidate at the maximum of the declarer's sum among the candidates alive at the end, with its discards; else
 *              exactly the list launch's (the Bot's exchange for a waiting game outside the set; -1 / 255).
 *   bids       sum_out [N,4,20] i32 (0 on the rows that are not played); count_out [N,4,20] i32 as above — row 19's is the end
 *              of its unit's last round; value_out [N,4,20] i32: 0 where the count is 0, else the nearest integer to sum x W /
 *              count, halves away from zero, in 64-bit integers — exactly sum x W / count where the count divides W.  value_out
 *              stands in for sum_out as the `sums` of tarok_bid_round / tarok_bid_round_pass at playouts = W.
 * Consequences: a one-round schedule (W) writes the _net_list launch's bytes at worlds = W, for every output, depth and
 * pass_value, with value_out = sum_out and count W on the live rows; and for any schedule a row whose count is e equals that
 * launch's row at worlds = e (all four columns, for the exchange).
 *
 * The launches (all on `stream`; no host read, no allocation, no synchronisation: capturable, the bids' first call
 * included): for the bids the deal; one init kernel (the on and alive words, the running sums and counts zeroed); then per
 * round the prefix sum over the units, the round's items — its worlds alone, under their true indices; every slot below the
 * round's total and none at or above it —, the playouts over a grid sized by the round's bound, and the sums with the
 * survivor rule, which writes the next on words (0 once one arm is left) and, on the last round, the outputs.
 *
 * The bounds, which the host computes without reading the env.  a_0 = 6 x D (exchange) or R = the rows of `contracts` (bids);
 * a_{r+1} = ceil(a_r / 2);
 *     exchange  B_r = n x a_r x W_r
 *     bids      B_r = n x U x (a_r + pass_value) x W_r, U = popc(seats) without seats_per_game, else 4
 * and B = max_r B_r sizes the four item arrays; the play grid of round r is B_r's.
 * scratch: device memory, 16-byte aligned, contents undefined afterwards.  With units = 6 n / 4 n:
 *     exchange  bytes = 48 x B + 20 x 6 n D + 12 x units + 4 x ceil(units / 256) + 4
 *     bids      bytes = 48 x B + 8 x 80 n + 40 n + 12 x units + 4 x ceil(units / 256) + 4
 * each rounded up to a multiple of 16 — the item arrays at B; a row's running sums and count; the bids' deal; the units' on,
 * alive and base words; the scan's partials and the total word, in that order.
 * tarok_playout_bids_net_halving_scratch_bytes takes the seat set the launch will get and per_game_seats = 1 where it will get
 * a seats_per_game array.
 * The _scratch_bytes entries return TAROK_EINVAL for a NULL env, a schedule outside the rules above, discard_sets outside
 * 1..TAROK_EXCHANGE_MAX_SETS, contracts outside 1..TAROK_BID_ALL_CONTRACTS, seats outside 0..15, per_game_seats or
 * pass_value outside 0..1, and a round bound that reaches 2^31 items.  The launches: TAROK_EINVAL (before any HIP call) for
 * all of those, for everything the _net_list launches refuse (net_seats outside 0..15, a NULL weight array, depth outside
 * 0..TAROK_PLAYOUT_FRONT_MAX_DEPTH, value_scale not finite or <= 0), a NULL or misaligned scratch, scratch_bytes below the
 * size, and every output NULL. */
int64_t tarok_playout_exchange_net_halving_scratch_bytes(const tarok_env *env, int rounds, const int *round_worlds,
                                                         int discard_sets);
int tarok_playout_exchange_net_halving(tarok_env *env, int rounds, const int *round_worlds, int discard_sets, uint64_t salt,
                                       int seats, const uint8_t *seats_per_game, int net_seats, int depth, float value_scale,
                                       const void *w1, const float *b1, const void *w2, const float *b2, const void *w3,
                                       const float *b3, void *scratch, int64_t scratch_bytes, int32_t *sum_out,
                                       int32_t *count_out, int8_t *choice_out, uint8_t *discards_out, void *stream);
int64_t tarok_playout_bids_net_halving_scratch_bytes(const tarok_env *env, int rounds, const int *round_worlds, int contracts,
                                                     int seats, int per_game_seats, int pass_value);
int tarok_playout_bids_net_halving(tarok_env *env, uint32_t episode, const uint8_t *deals, int rounds, const int *round_worlds,
                                   int contracts, uint64_t salt, int seats, const uint8_t *seats_per_game, int net_seats,
                                   int depth, float value_scale, int pass_value, const void *w1, const float *b1,
                                   const void *w2, const float *b2, const void *w3, const float *b3, void *scratch,
                                   int64_t scratch_bytes, int32_t *sum_out, int32_t *count_out, int32_t *value_out,
                                   void *stream);

/* The learner's network input for a minibatch: features_out[j] [256] bf16 (0.0 / 1.0) = the bits
 * of feature_words[index[j]] (feature_words [M,4] u64 as written by feature_words_out; index
 * [n_samples] i64 sample numbers, or NULL for samples 0..n_samples-1).  Gather + expansion in one
 * pass. */
int tarok_expand_features(tarok_env *env, int64_t n_samples, const uint64_t *feature_words,
                          const int64_t *index, void *features_out, void *stream);

/* The learner's loss for the policy above, forward and gradient in one pass: clipped-surrogate
 * policy loss + value loss - entropy bonus over the LEGAL cards of every sample (build-owned:
 * the reference has no policy-gradient learner).
 *   out_bf16 [B,64] bf16 head outputs (0..53 card logits, 54 value), obs [B] observation words
 *   (legal mask), action [B] i64 the card played, logp_old [B] f32 its log-probability at play
 *   time, advantage / ret / weight [B] f32 (weight 0: sample ignored);
 *   loss = sum_i w_i (-min(r_i A_i, clamp(r_i, 1-clip, 1+clip) A_i) + vf (v_i - ret_i)^2 - ent H_i)
 *          * inv_weight_sum[0] (a device scalar, so that no host round trip sits between the
 *          minibatch's weight sum and this launch),   r_i = exp(logp_i[a_i] - logp_old_i), H_i the
 *          entropy of the masked softmax;
 *   dout_bf16 [B,64] bf16 = d loss / d out;  partial_out [ceil(B/256),4] f32 = per-workgroup sums of
 *   {w pi, w (v-ret)^2, w H, 0} (sum them for the loss terms). */
int tarok_ppo_loss(tarok_env *env, int64_t n_samples, const void *out_bf16, const uint64_t *obs,
                   const int64_t *action, const float *logp_old, const float *advantage, const float *ret,
                   const float *weight, float clip, float vf_coef, float ent_coef, const float *inv_weight_sum,
                   void *dout_bf16, float *partial_out, void *stream);

/* The reference agent's training targets in its own form (Nevronski_igralec.rezultat_stiha +
 * rezultat_igre, Igralec.py:387-446) for a recorded rollout of T lock-steps, T a multiple of 4, started on a trick
 * boundary (trick b = rows 4b .. 4b+3 of every slot, through the auto-resets):
 *   obs_before [T,N] u64   the observation word each card was chosen on (legal mask = `mozne`, seat to move)
 *   action [T,N] u8, trick [T,N] u16 (trick_out), done [T,N] u8, reward [T,N,4] i16 with TAROK_REWARD_REF
 *   next_q [T,N] f32 or NULL  the agent's own next_Q_max at each decision (Igralec.py:351); NULL = 0
 *   dy_out [T/4,N,4,54] f32: per (trick, game, seat) -70 on the cards that were not legal (:392-393), on the card
 *           played +/- Roka.vrednost_stiha(trick) by who took it (:412-416) + final_reward_factor * next_max (:441),
 *           next_max = next_q at the seat's next decision (:417-418) or the final reward on the game's last trick (:439)
 *   meta_out [T/4,N,4] u8: bit 0 row valid (the seat played in a completed trick), bit 1 last transition of its
 *           game, bit 2 the seat's next decision lies beyond the rollout (next_max taken as 0).
 * Parity unpinned for the assembly (no reference fixture; Igralec.py cannot be imported), pinned for its inputs. */
int tarok_targets_ref(tarok_env *env, int T, const uint64_t *obs_before, const uint8_t *action, const uint16_t *trick,
                      const uint8_t *done, const int16_t *reward, const float *next_q, float final_reward_factor,
                      float *dy_out, uint8_t *meta_out, void *stream);

/* ---- The learner's update of the policy above as a few fused launches (build-owned, like the policy itself:
 * the reference's learner is a double-Q LSTM agent under pytorch-lightning, Igralec.py:545-714).  The network
 * 256-256-256-64 lives in ONE flat f32 vector of TAROK_MLP_PARAMS entries, in torch.nn.Linear layouts:
 * W1 [256,256] | b1 [256] | W2 [256,256] | b2 [256] | W3 [64,256] | b3 [64]  (offsets TAROK_MLP_*). */
#define TAROK_MLP_W1 0
#define TAROK_MLP_B1 65536
#define TAROK_MLP_W2 65792
#define TAROK_MLP_B2 131328
#define TAROK_MLP_W3 131584
#define TAROK_MLP_B3 147968
#define TAROK_MLP_PARAMS 148032
#define TAROK_LEARN_PAD 256 /* padding rows of the activation arrays of tarok_learn_chain / tarok_learn_dw */
#define TAROK_LEARN_MAX_BATCH 4194048 /* samples per minibatch of tarok_learn_dw (its arrays are addressed through 32-bit
                                       * byte offsets: (B + 255) * 512 < 2^31); larger: TAROK_EINVAL */

/* Returns of a rollout of T lock-steps (rows [T,N] as written by tarok_policy_step): every card is credited with
 * its seat's final score of the game it belongs to, times reward_scale.
 *   rec_out [T,N,4] f32: {log-probability at play time, return, value at play time, bits: card | known << 8}
 *           (known = that game ended inside the rollout; other samples carry weight 0 in the update)
 *   stats_out [4] f32: {mean, 1 / std of the advantages (return - value) over the known samples, known fraction, 0}
 *   scratch [ceil(N/256),4] f32. */
int tarok_learn_returns(tarok_env *env, int T, const uint8_t *done, const int16_t *reward, const uint64_t *obs,
                        const float *logp, const float *value, const uint8_t *action, float reward_scale,
                        float *rec_out, float *stats_out, float *scratch, void *stream);

/* The same record with returns by GAE(gamma, lambda) per seat, bootstrapped from the value of the SAME seat's next
 * decision inside the rollout (arrays as tarok_learn_returns).  Per slot, backwards over t = T-1 .. 0, with a state per
 * seat s (have[s] = false at first):
 *   done[t]:  for every seat s: pend_r[s] = reward[t][s] * reward_scale, next_v[s] = next_adv[s] = 0, have[s] = true
 *   s = the seat to move in obs[t], v = value[t];
 *     have[s]:   delta = pend_r[s] + gamma * next_v[s] - v,  A = delta + gamma * lambda * next_adv[s],  known = 1
 *     otherwise: A = 0, known = 0
 *   return = A + v;  then next_v[s] = v, next_adv[s] = A, pend_r[s] = 0, have[s] = true
 * gamma discounts per decision of the seat (its cards lie four lock-steps apart), not per lock-step.  With gamma =
 * lambda = 1 the return of every sample tarok_learn_returns knows equals that one's (up to f32 rounding of the sum).
 *   known = the seat moves again, or its game ends, inside the rollout: only a seat's LAST decision of a game still
 *           unfinished at the end of the rollout is unknown (weight 0; it still serves as the bootstrap of the seat's
 *           earlier decisions) — at most 4 samples per slot, so stats_out[2] >= 1 - 4 / T for rollouts whose slots
 *           are never idle (auto-reset).
 *   stats_out: over the known samples, of A.  Bit-reproducible from call to call (fixed summation order).
 * gamma or lambda outside [0, 1] or NaN: TAROK_EINVAL. */
int tarok_learn_returns_gae(tarok_env *env, int T, const uint8_t *done, const int16_t *reward, const uint64_t *obs,
                            const float *logp, const float *value, const uint8_t *action, float reward_scale, float gamma,
                            float lambda, float *rec_out, float *stats_out, float *scratch, void *stream);

/* tarok_learn_returns (gae = 0; gamma and lambda are ignored) or tarok_learn_returns_gae (gae = 1; its checks of gamma
 * and lambda) for a rollout in which only some seats are the learner's: training against a frozen opponent seated by
 * tarok_policy_step_versus.
 *   seats, seats_per_game   exactly as in tarok_policy_step_versus: `seats` is a 4-bit set used for every slot when
 *                           seats_per_game is NULL, seats_per_game [N] u8 one set per slot (bits 4..7 ignored); bit s
 *                           set = seat s is the learner's.  A slot keeps its set through the auto-resets.
 * The record differs in `known` alone: the unmasked walk's known AND (the seat to move in obs[t] is in the slot's set).
 * logp, return, value and the card byte are written for every sample as before, and the per-seat GAE state is updated
 * for every seat as before: a seat's chain only ever reads that seat's own values, so a learner seat's returns equal
 * the unmasked ones.
 *   stats_out = {mean, 1 / std of the advantages over the known samples, known / (T N), 0}, in the fixed summation
 *   order of the kernels it extends (bit-reproducible).  No known sample at all: {0, 1e6, 0, 0}.
 * With seats = 15 and seats_per_game = NULL, rec_out and stats_out are byte for byte those of tarok_learn_returns
 * (gae = 0) / tarok_learn_returns_gae (gae = 1).  rec_out, stats_out, scratch as in tarok_learn_returns.
 * TAROK_EINVAL (before any HIP call) for a NULL env or required array, T < 1, seats outside 0..15, gae outside {0, 1}
 * and, with gae = 1, gamma or lambda outside [0, 1] or NaN. */
int tarok_learn_returns_seats(tarok_env *env, int T, const uint8_t *done, const int16_t *reward, const uint64_t *obs,
                              const float *logp, const float *value, const uint8_t *action, float reward_scale, int gae,
                              float gamma, float lambda, int seats, const uint8_t *seats_per_game, float *rec_out,
                              float *stats_out, float *scratch, void *stream);

/* Stable compaction of the known samples of a record: index_out[0 .. count) = the sample numbers j in [0, M) whose
 * known bit (bit 8 of rec[j].w) is set, in ascending order, count_out[0] (device) = how many there are.  Entries of
 * index_out at and beyond count are NOT written.  Deterministic: the same input gives the same bytes.  The list is what
 * tarok_learn_chain takes as `index`: minibatches drawn from it hold known samples only, so a learner that owns one
 * seat of four does not run the forward, loss and backward of the other three (they would carry weight 0).
 *   rec [M,4] f32 (tarok_learn_returns*), index_out [M] i64, scratch: tarok_learn_select_scratch_bytes(M) bytes,
 *   16-byte aligned.  M up to 2^28 and beyond: sample numbers and byte offsets are 64 bit.
 * Three small stream-ordered launches (count per tile of TAROK_LEARN_SELECT_TILE samples, scan of the tile counts,
 * scatter); no workgroup waits for another.  TAROK_EINVAL for a NULL env or pointer, or M < 1. */
#define TAROK_LEARN_SELECT_TILE 2048 /* samples one workgroup of the scatter launch handles */
int64_t tarok_learn_select_scratch_bytes(int64_t M);
int tarok_learn_select(tarok_env *env, int64_t M, const float *rec, int64_t *index_out, int64_t *count_out,
                       void *scratch, void *stream);

/* Forward, loss and backward chain of one minibatch of B samples (sample j = row index[j] of feature_words [M,4] /
 * rec [M,4]; index NULL: row j): feature gather + expansion -> layers 1-3 -> the loss of tarok_ppo_loss (advantage
 * = (return - value - stats[0]) * stats[1], weight = known) -> dH2, dH1.  Weights: the bf16 fragment-order copies
 * tarok_learn_adam writes (w3t / w2t: of the transposes), biases: pointers into the flat vector.
 *   Xw [B + TAROK_LEARN_PAD, 4] u64: the samples' feature words in minibatch order (layer 1's input for tarok_learn_dw);
 *   H1 / H2 / dH2 / dH1 [B + TAROK_LEARN_PAD, 256] bf16, dOut [B + TAROK_LEARN_PAD, 64] bf16 (rows B.. are padding that
 *   tarok_learn_dw may read and ignores; values unscaled: weight w, not w / sum w);
 *   scratch [ceil(B/96),4] f32; terms_out [4] f32 = {policy loss, value loss, entropy (weighted means),
 *   1 / max(sum w, 1)}; running [4] f32 or NULL: += {the three terms, 1}. */
int tarok_learn_chain(tarok_env *env, int64_t B, const uint64_t *feature_words, const int64_t *index, const float *rec,
                      const float *stats, float clip, float vf_coef, float ent_coef, const void *w1, const float *b1,
                      const void *w2, const float *b2, const void *w3, const float *b3, const void *w3t, const void *w2t,
                      uint64_t *Xw, void *H1, void *H2, void *dOut, void *dH2, void *dH1, float *scratch, float *terms_out,
                      float *running, void *stream);

/* tarok_learn_chain with a distillation term: the cross-entropy of the policy against a target row per sample (the
 * playout teacher's: tarok_playout_targets), beside the clipped surrogate, the value loss and the entropy bonus.
 * target [M,64] bf16, row = sample number as for rec (gathered through index).  Per sample i, weight w_i (the known bit):
 * p = the masked softmax of the loss, q_c = the row's value at legal card c — columns of illegal cards and 54..63 are
 * dropped by a select (a NaN there reaches no output), a sample without a legal card has none —, S_i = sum_c q_c:
 *     ce_i = -sum_c q_c log p_c
 *     loss            += distill_coef * sum_i w_i ce_i / max(sum w, 1)
 *     d loss / d logit_c += distill_coef * w_i (S_i p_c - q_c)   on the legal cards; unscaled in dOut like the other parts
 * S_i p_c - q_c is the exact gradient of ce_i for q as stored (bf16 rows do not sum to exactly 1).  A zero row adds nothing.
 *   distill_scratch [ceil(B/96),2] f32; distill_out [2] f32 = {sum w ce, sum w S} / max(sum w, 1), summed in a fixed
 *   order (bit-reproducible); distill_running [2] f32 or NULL: += distill_out.
 * Every other argument and output as in tarok_learn_chain: H1, H2 and terms_out are those of tarok_learn_chain on the
 * same inputs, and distill_coef = 0 leaves dOut equal to its dOut.  tarok_learn_dw / tarok_learn_adam read dOut and
 * terms[3] as before.  TAROK_EINVAL as tarok_learn_chain, and for a NULL target, distill_scratch or distill_out or a
 * distill_coef that is NaN or infinite. */
int tarok_learn_chain_distill(tarok_env *env, int64_t B, const uint64_t *feature_words, const int64_t *index, const float *rec,
                              const float *stats, float clip, float vf_coef, float ent_coef, const void *w1, const float *b1,
                              const void *w2, const float *b2, const void *w3, const float *b3, const void *w3t,
                              const void *w2t, uint64_t *Xw, void *H1, void *H2, void *dOut, void *dH2, void *dH1,
                              float *scratch, float *terms_out, float *running, const void *target, float distill_coef,
                              float *distill_scratch, float *distill_out, float *distill_running, void *stream);

/* The weight and bias gradients of that minibatch: grad_out [TAROK_MLP_PARAMS] f32 = terms[3] * (dH^T H per layer,
 * column sums of dH), in the flat parameter order.  workspace: tarok_learn_workspace_bytes(env) bytes.
 * B <= TAROK_LEARN_MAX_BATCH. */
int64_t tarok_learn_workspace_bytes(tarok_env *env);
int tarok_learn_dw(tarok_env *env, int64_t B, const uint64_t *Xw, const void *H1,
                   const void *H2, const void *dOut, const void *dH2, const void *dH1, const float *terms,
                   void *workspace, float *grad_out, void *stream);

/* Gradient-norm clip (max_norm <= 0: none) + Adam (torch.optim.Adam semantics) on the flat vectors, then the
 * kernels' bf16 fragment-order weight copies (any may be NULL).  step: device counter, incremented.
 * apply = 0: only rebuild the copies from param.  gnorm_out [1] f32 or NULL. */
int tarok_learn_adam(tarok_env *env, float *param, const float *grad, float *m, float *v, int32_t *step, float lr,
                     float beta1, float beta2, float eps, float max_norm, void *w1, void *w2, void *w3, void *w3t,
                     void *w2t, float *gnorm_out, int apply, void *stream);

/* Diagnostics: when `stamps` (device, [ceil(N/64), 3] u64) is non-NULL every wave of the step
 * kernels records {s_memrealtime at entry, at exit, shader cycles in between}.  NULL turns it off. */
int tarok_debug_stamps(tarok_env *env, uint64_t *stamps);
/* The same with the buffer's capacity in 64-bit words stated: a kernel writes its stamps only into a buffer that
 * holds all of them — the step kernels 3 per wave (3 * ceil(N/64)), tarok_policy_mlp and tarok_learn_chain 8 per
 * workgroup (8 * ceil(N/128), 8 * ceil(B/96)).  tarok_debug_stamps registers the step kernels' size. */
int tarok_debug_stamps_sized(tarok_env *env, uint64_t *stamps, int64_t n_words);
/* Self-test of the refill role as the step kernels compile it (tests only; it takes over the env's refill lists and
 * next-game lines and leaves them empty: tarok_reset before the env is used again).  Every group's lists are filled by
 * hand — every slot, episodes episode0+1 .. episode0+per_slot (1..14), in list order `order` (0 ascending slots, 1
 * descending, 2 scattered) — `reps` step launches of `kind` (0 tarok_step_random, 1 tarok_policy_random + tarok_step,
 * 2 tarok_krog_random of 4 cards, 3 of 2 cards) work them off, and every line is compared with a re-deal by a kernel
 * of its own.  report_out (host, 49 u64): [0] lines that differ, then {slot, episode, play word read / expected, seat
 * word read / expected} of the first eight.  It expects the Bot's lines: it is not meaningful on an env whose lines
 * tarok_front_lines has rewritten. */
int tarok_debug_refill_selftest(tarok_env *env, int kind, int per_slot, uint32_t episode0, int order, int reps, uint64_t *report_out);

/* Canonical state for parity checks / checkpoints: lanes_out [10,N] u64. */
int tarok_get_state(tarok_env *env, uint64_t *lanes_out, void *stream);
/* Restore every game from canonical lanes (the inverse of tarok_get_state): checkpoint/resume,
 * or hand-built positions.  The RNG keys / episode numbers / next-game buffers are untouched. */
int tarok_set_state(tarok_env *env, const uint64_t *lanes_in, void *stream);
/* Per-slot bookkeeping: episode_out [N] u32 (current episode number),
 * score_sum_out [N,4] i32 (scores summed over the slot's finished games =
 * Tarok.rezultati per seat, Tarok.py:59-61).  Either may be NULL. */
int tarok_get_counters(tarok_env *env, uint32_t *episode_out, int32_t *score_sum_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
