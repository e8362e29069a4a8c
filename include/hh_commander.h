/*
 * hh_commander.h — C ABI of the TRAINABLE commander policy of train_hier.py (part of libhh_world.so).
 *
 * What RLlib's sampler evaluates per commander step for every agent of a 3-vs-3 HighLevelEnv arena (train_hier.py:100-165 with
 * models/ac_models_hier.py:70-112 CommanderGru): the actor (three input FCs on column ranges of the own 34-wide observation, a
 * fourth FC on all of it, one step of a 200-wide GRU, normalize(x_full + y), the module-level shared layer, 3 logits), the
 * Categorical draw and its log-probability, and the value branch (v1..v3 on [obs_k | act_k] of the own and the two other agents
 * in ascending id, v4 on all three, its own GRU, the same shared layer, val_out).  Both GRU states are per agent row and are
 * carried by the caller: h_in / h_out [rows, 2, 200], state 0 = rnn_act, state 1 = rnn_val (get_initial_state order).
 * One fused gfx950 kernel over rows = 3 x n_arenas agent rows (hh_commander_kernel.h).
 *
 * Conventions as in hh_abi.h: 0 on success or a negative HH_E_* code, never throws; [dev] = caller-owned device memory,
 * [host] = host memory; `stream` is a hipStream_t passed as void*.
 */
#ifndef HH_COMMANDER_H
#define HH_COMMANDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HH_CMD_OBS 34     /* commander observation width (env_hier.py: 14 + 10 N_OPP_HL) */
#define HH_CMD_AGENTS 3   /* agent rows per arena (central_critic_observer hard-codes three) */
#define HH_CMD_HIDDEN 200 /* GRU width of both branches */
#define HH_CMD_ACTIONS 3  /* Discrete(N_OPP_HL + 1) */
#define HH_CMD_LOGITS 4   /* row width of the optional logits output (zero padded) */

typedef struct hh_commander hh_commander;

/* [host] fp32, row-major [out, in] as the reference's state_dict() holds them */
typedef struct hh_commander_weights {
    const float *inp_w[4], *inp_b[4];                       /* inp1 [50,4]  inp2 [200,20]  inp3 [50,10]  inp4 [200,34] */
    const float *act_w_ih, *act_w_hh, *act_b_ih, *act_b_hh; /* rnn_act.{weight,bias}_{ih,hh}_l0  [600,200] [600], gate rows r|z|n */
    const float *shared_w, *shared_b;                       /* shared_layer._model.0  [500,500] [500]  (one tensor, both branches) */
    const float *act_out_w, *act_out_b;                     /* [3,500] [3] */
    const float *v_w[4], *v_b[4];                           /* v1..v3 [100,35]  v4 [200,105] */
    const float *val_w_ih, *val_w_hh, *val_b_ih, *val_b_hh; /* rnn_val.* */
    const float *val_out_w, *val_out_b;                     /* [1,500] [1] */
} hh_commander_weights;

/* a commander network on `device`; max_rows = the largest 3 x n_arenas hh_commander_sample will be given */
int hh_commander_create(int device, int32_t max_rows, hh_commander **out);
int hh_commander_destroy(hh_commander *c);

/* load (or replace) the weights from [host] arrays: staged in a temporary device buffer and packed there into the kernel's split-fp16
 * fragment layout by the kernel hh_commander_refresh_weights launches (csrc/hh_weight_refresh.h), after the destination is cleared.
 * Synchronous: the packed bytes are in place when the call returns, the arrays may be freed or overwritten, and a launch issued
 * afterwards on any stream sees the new weights.  An invalid argument (HH_E_ARG) or a failed staging (HH_E_HIP) changes nothing. */
int hh_commander_set_weights(hh_commander *c, const hh_commander_weights *w);

/* The learner's new weights without a host round trip (csrc/hh_weight_refresh.h): the same struct with [dev] fp32 pointers in the same
 * layout; what hh_commander_set_weights writes is rewritten in place with the same bytes (fp16 planes, fp32 section; the GRU bias sums
 * b_ih + b_hh are fp32 adds) by the same kernel, one launch ordered on `stream`: no host synchronisation, no allocation, graph-capturable,
 * device addresses unchanged.  HH_E_ARG, nothing enqueued: no weights loaded yet, or a missing pointer. */
int hh_commander_refresh_weights(hh_commander *c, const hh_commander_weights *w, void *stream);
/* Test hook: one packed part (HH_COMMANDER_PART_*) to dst [dev] (cap bytes) on `stream`; *bytes = its size (dst == NULL: the size only) */
#define HH_COMMANDER_PART_PLANES 0 /* (hi, lo) fp16 fragment planes */
#define HH_COMMANDER_PART_F32 1    /* biases, GRU bias sums, output layers (fp32) */
int hh_commander_copy_packed(hh_commander *c, int32_t part, void *dst, int64_t cap, int64_t *bytes, void *stream);

/* One sampler step of every agent row (row r = agent slot r % 3 of arena r / 3):
 *   obs       [dev] f32 [N, 3, 34]      the commander observations hh_hl_end / hh_reset write (dead agents: zero rows)
 *   h_in      [dev] f32 [3N, 2, 200]    the GRU states the forward uses; rows of arenas flagged fresh are OVERWRITTEN with zeros (the
 *                                       stored state_in is then exactly what the forward used)
 *   h_out     [dev] f32 [3N, 2, 200]    the new states (state_out); must not overlap h_in (HH_E_ARG)
 *   fresh     [dev] u8  [N] or NULL     non-zero: the arena starts an episode at this step (get_initial_state: zero states)
 *   w         the world whose agents these are (n_arenas == its arena count), or NULL.  With a world, agent slot i of arena n draws
 *             u = U(seed, arena_offset + n, episode, steps, i + 1, HH_SITE_COMMANDER_SAMPLE, 0)  (hh_rng.h) with the arena's CURRENT
 *             counters, as hh_policy_sample does.
 *   uniforms  [dev] f64 [3N] or NULL    overrides the keyed draw.  Exactly one of w / uniforms unless greedy.
 *   crit_act  [dev] f32 [N, 3] or NULL  the value branch's act_k inputs per agent slot (on_postprocess_trajectory's action / 2); NULL =
 *                                       zeros, which is what the sampler sees
 *   greedy    != 0: arg-max instead of a draw (logp is then the log-probability of the arg-max)
 *   actions   [dev] i8  [N, 3]          the layout hh_hl_begin / hh_hl_begin_variants read
 *   logp      [dev] f32 [N, 3]
 *   vf        [dev] f32 [N, 3]          value_function(); nullable (the value GRU state still advances)
 *   logits    [dev] f32 [3N, 4]         nullable (4-byte alignment suffices)
 * Inverse CDF as hh_policy_sample: m = max l, S = sum exp(l_i - m) in index order, t = (float)u * S, the action is the first i whose
 * running sum exceeds t (the last if none does); logp = (l_a - m) - log S.  Everything is ordered on `stream`; no host synchronisation
 * and no allocation (HIP-graph capturable). */
struct hh_world;
int hh_commander_sample(hh_commander *c, const float *obs, int32_t n_arenas, float *h_in, float *h_out, const uint8_t *fresh,
                        struct hh_world *w, const double *uniforms, const float *crit_act, int32_t greedy, int8_t *actions, float *logp,
                        float *vf, float *logits, void *stream);

/* name of the kernel a call of n_arenas arenas launches, as a profiler prints it */
int hh_commander_kernel_name(hh_commander *c, int32_t n_arenas, char *buf, int32_t len);

/* evaluation.py:40-48 for every arena: per commander step the actor of CommanderGru over agent slots 0..n_agents-1 in order, slot 0
 * from zero rnn_act state, slot k from slot k-1's state_out (the reference resets states = [zeros(200), zeros(200)] at the start of
 * every step and threads each agent's state_out into the next agent's state_in); greedy first arg-max (explore = False).  No value
 * branch: evaluation never reads it.  Every link's logits equal, bit for bit, what hh_commander_sample gives for the same row and h_in.
 *   obs     [dev] f32 [N, n_agents, 34]   dead agents: the zero rows hh_hl_end writes
 *   actions [dev] i8  [N, n_agents]       the layout hh_hl_begin / hh_hl_begin_variants read
 *   h_out   [dev] f32 [N, n_agents, 200]  nullable: rnn_act state after each link (test hook)
 *   logits  [dev] f32 [N, n_agents, 4]    nullable (zero padded like hh_commander_sample's)
 * 1 <= n_agents <= 5 and n_arenas x n_agents <= max_rows of hh_commander_create; stream-ordered, no host sync, no allocation,
 * graph-capturable. */
int hh_commander_act_chain(hh_commander *c, const float *obs, int32_t n_arenas, int32_t n_agents, int8_t *actions, float *h_out,
                           float *logits, void *stream);
/* name of the kernel hh_commander_act_chain launches, as a profiler prints it */
int hh_commander_chain_kernel_name(hh_commander *c, int32_t n_arenas, int32_t n_agents, char *buf, int32_t len);

/* Whole-episode GRU-sequence batches of the commander (batch_mode = "complete_episodes" with a recurrent model, train_hier.py:182):
 * what hh_episodes_emit (hh_abi.h) does for PPORollout, plus RLlib's cut of every agent's trajectory into sequences of at most
 * max_seq_len (L) steps, each with the GRU states of its first step.  hh_commander_episodes_emit takes one collect's [T, N, ...]
 * buffers (auto-resetting arenas: the row after a done is the next episode's row 0), keeps every arena's running episode in a
 * device-side carry across calls — its rows, and the GRU states at its sequence starts (within-episode steps 0, L, 2L, ...) only —
 * and writes every episode that ended in this window into one flat batch, arena-major, then episode, then time; its sequences
 * (ceil(E / L) per episode of E rows: L, ..., L, then the remainder) in the same order; and o_state_in[s] = state_in of the
 * sequence's first step, bit for bit.  adv / target: hh_gae_rllib's recursion over each whole episode with last_r = 0.0.
 * Launches on the calling thread's current device, which must own every buffer; no host synchronisation and no allocation
 * (graph-capturable).  All pointers [dev].
 * Capacities (checked): carry_cap >= the rows an unfinished episode can have; row_cap >= N (carry_cap + T); ep_cap >= N T;
 * seq_cap >= N (T + carry_cap / L) (an arena emits at most carry_cap + T rows in at most T episodes, and sum ceil(E_k / L) <=
 * n_eps + (rows - n_eps) / L).  If an episode outgrows the carry anyway, counts[2] is set (sticky) and nothing is written out of
 * bounds.  The caller zeroes carried / episode (and counts) before the first call and whenever its arenas are reset. */
typedef struct hh_commander_episode_bufs {
    int32_t T;                /* commander steps per call */
    int32_t N;                /* arenas */
    int32_t max_seq_len;      /* L >= 1 */
    int32_t carry_cap;        /* rows per arena the carry holds */
    int64_t row_cap;          /* rows of every output column (>= N (carry_cap + T); < 2^31) */
    int64_t ep_cap;           /* entries of the episode table (>= N T) */
    int64_t seq_cap;          /* entries of the sequence table and of o_state_in (>= N (T + carry_cap / L)) */
    double gamma;
    double lam;
    /* one collect (read): obs f32 [T+1, N, 3, 34], actions i8 [T, N, 3], logp f32 [T, N, 3], vf f32 [T+1, N, 3], reward f32 [T, N, 3],
       valid u8 [T, N, 3], done u8 [T, N], state_in f32 [T+1, N, 3, 2, 200] (16-byte aligned) */
    const float *obs;
    const int8_t *actions;
    const float *logp;
    const float *vf;
    const float *reward;
    const uint8_t *valid;
    const uint8_t *done;
    const float *state_in;
    /* carry (read and written): the same row columns [N, carry_cap, ...], c_state f32 [N, ceil(carry_cap / L), 3, 2, 200] (16-byte
       aligned: the states at the running episode's sequence starts), carried / episode i32 [N] (rows held; episodes finished since the
       reset), scratch i32 [10 N + 4] */
    float *c_obs;
    int8_t *c_actions;
    float *c_logp;
    float *c_vf;
    float *c_reward;
    uint8_t *c_valid;
    float *c_state;
    int32_t *carried;
    int32_t *episode;
    int32_t *scratch;
    /* batch (written): the collect's row columns [row_cap, ...], adv / target f32 [row_cap, 3], done u8 [row_cap] (1 on an episode's
       last row only), arena / episode / t i32 [row_cap]; episode table [ep_cap]; sequence table [seq_cap]: first row in the batch,
       length, episode entry; o_state_in f32 [seq_cap, 3, 2, 200] (16-byte aligned) */
    float *o_obs;
    int8_t *o_actions;
    float *o_logp;
    float *o_vf;
    float *o_reward;
    uint8_t *o_valid;
    float *o_adv;
    float *o_target;
    uint8_t *o_done;
    int32_t *o_arena;
    int32_t *o_episode;
    int32_t *o_t;
    int32_t *ep_start;
    int32_t *ep_len;
    int32_t *ep_arena;
    int32_t *seq_start;
    int32_t *seq_len;
    int32_t *seq_ep;
    float *o_state_in;
    int32_t *counts;          /* [4]: rows, episodes written by this call; overflow flag (sticky); sequences written by this call */
} hh_commander_episode_bufs;

int hh_commander_episodes_emit(const hh_commander_episode_bufs *b, void *stream);

/* hh_commander_episodes_emit with one optional per-agent float column (hh_episode_aux, hh_abi.h: aux [T, N, 3, aux_dim], c_aux
 * [N, carry_cap, 3, aux_dim], o_aux [row_cap, 3, aux_dim]) that moves with the rows; x = NULL: hh_commander_episodes_emit exactly. */
struct hh_episode_aux;
int hh_commander_episodes_emit_aux(const hh_commander_episode_bufs *b, const struct hh_episode_aux *x, void *stream);

/* hh_commander_episodes_emit_aux (x = NULL: no aux column) that appends to the batch in place until it holds at least train_rows rows:
 * hh_episodes_emit_append of hh_abi.h (acc i32 [HH_EP_ACC], totals NULL or i64 [2]; the same rules and errors), with the sequences:
 * acc[3] is the sequence base, seq_start / seq_ep are absolute positions in the accumulated batch, and seq_cap is the accumulated
 * batch's capacity (train_rows - 1 + N (T + carry_cap / L) never overflows: one-row episodes cost a sequence each). */
int hh_commander_episodes_emit_append(const hh_commander_episode_bufs *b, const struct hh_episode_aux *x, int64_t train_rows,
                                      int32_t *acc, int64_t *totals, void *stream);

/* Complete snapshot of a commander net (checkpointing; csrc/hh_snapshot.h, conventions of hh_world_snapshot in hh_abi.h): the packed
 * weights exactly as the kernels read them (HH_COMMANDER_PART_PLANES, then HH_COMMANDER_PART_F32) in one section behind the 208-byte
 * header (magic "HHSC", format version 1, digest of the geometry constants and the section size, N = 0, A = HH_CMD_AGENTS, slot count 1,
 * layout word [0] = weights loaded).  hh_commander_restore checks the whole header first (HH_E_ARG, nothing written: another version or
 * geometry, a net without weights on one side only, a short buffer) and writes in place: load the receiving net once with
 * hh_commander_set_weights.  Copies only; both calls synchronise `stream`. */
int hh_commander_snapshot_bytes(hh_commander *c, int64_t *bytes);
int hh_commander_snapshot(hh_commander *c, void *host_buf, int64_t bytes, void *stream);
int hh_commander_restore(hh_commander *c, const void *host_buf, int64_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HH_COMMANDER_H */
