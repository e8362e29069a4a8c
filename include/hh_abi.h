/*
 * hh_abi.h — C ABI of the MI355X batched air-combat world (libhh_world.so).
 *
 * The reference has no FFI: its boundary is RLlib's Python MultiAgentEnv protocol
 * (envs/env_hetero.py:20-63 LowLevelEnv, envs/env_hier.py:27-47 HighLevelEnv,
 * envs/env_base.py:62-109 reset/step).  This header is what a binding for that boundary
 * binds to; hhmarl_2d_amd/{env_hetero,env_hier}.py are the ctypes bindings that re-expose the
 * reference's dict protocol on top of it (INTEGRATION.md shows the stub).
 *
 * Conventions: every function returns 0 on success or a negative HH_E_* code and never throws.
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  Every call that launches or copies makes the
 * world's device current for its duration and restores the caller's current device before it returns.  Buffers marked [dev] are
 * caller-owned device memory (e.g. torch tensors); [host] are host memory.  One host thread per
 * world.  The world owns only its struct-of-arrays state.
 *
 * Units are addressed 1..A in the reference (agents 1..n_agents, opponents after); arrays here
 * are 0-based slots in the same order.  A HighLevelEnv world has A = 6 unit slots, or A = 10 when a side has more than 3 aircraft
 * (HH_HL_SLOTS of hh_spec.h; up to 5 per side): with fewer aircraft than slots (n-vs-m evaluation scenarios) the slots behind the
 * last opponent are never alive and their rows read as zeros.
 */
#ifndef HH_ABI_H
#define HH_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HH_OK 0
#define HH_E_ARG (-1)      /* bad argument / unsupported configuration */
#define HH_E_HIP (-2)      /* HIP runtime error (hh_last_error() has the text) */
#define HH_E_NODEV (-3)    /* no usable GPU */

/* replaces the fields envs read from config.py's Namespace (config.py:17-54, 94-107) */
typedef struct hh_config {
    int32_t n_arenas;         /* arenas held by THIS world (this rank's shard) */
    int32_t env_kind;         /* HH_ENV_LOWLEVEL | HH_ENV_HIGHLEVEL */
    int32_t n_agents;         /* args.num_agents (2 low level; 1..5 high level) */
    int32_t n_opps;           /* args.num_opps   (2 low level; 1..5 high level: evaluation.py's n-vs-m scenarios) */
    int32_t level;            /* args.level 1..5 */
    int32_t agent_mode;       /* HH_MODE_FIGHT | HH_MODE_ESCAPE (args.agent_mode) */
    int32_t horizon;          /* args.horizon */
    int32_t friendly_kill;    /* args.friendly_kill */
    int32_t friendly_punish;  /* args.friendly_punish */
    int32_t esc_dist_rew;     /* args.esc_dist_rew */
    int32_t hier_action_assess;   /* args.hier_action_assess */
    int32_t hier_opp_fight_ratio; /* args.hier_opp_fight_ratio [%] */
    int32_t auto_reset;       /* 1: a finished arena is re-sampled inside hh_step */
    int32_t ext_opp_actions;  /* 1: opponents take actions from the caller (levels 4-5 frozen policies) */
    int32_t opp_side_selector; /* HighLevelEnv, evaluation.py with eval_hl = False: the opponents fly their OWN fight policies
                                  ("fight_{1,2}_opp" = L{eval_level_opp}, env_base.py:343-346,387-390): pilot_mode of an opponent's
                                  fight row carries HH_SEL_OPP_SIDE on top of policy type | aircraft type << 2 */
    int32_t reserved0;        /* keeps the doubles 8-byte aligned; must be 0 (hh_world_create refuses anything else: a caller built against the
                                 layout before opp_side_selector was added would otherwise be misread silently) */
    double map_size;          /* args.map_size */
    double glob_frac;         /* args.glob_frac */
    double rew_scale;         /* args.rew_scale */
    uint64_t seed;            /* keyed-RNG seed (hh_rng.h) */
    uint64_t arena_offset;    /* global id of local arena 0 (rank * n_arenas when sharded) */
} hh_config;

/* World snapshot used by hh_get_state / hh_set_state (parity tests, golden injection,
 * checkpointing).  All arrays are [host], arena-major: index = (arena * A + slot) * K + k. */
#define HH_ACF_K 6  /* lat, lon, hdg, spd, cmd_hdg, cmd_spd                       (a1, a6) */
#define HH_ACI_K 10 /* alive, ac_type, cannon_remain, cannon_burst, cannon_max,
                       missile_remain, rocket_max, missile_wait, has_missile, target      */
#define HH_RKF_K 4  /* lat, lon, hdg, cmd_hdg                                     (a10)   */
#define HH_RKI_K 4  /* alive, target, life, seq                                           */
#define HH_ARI_K 6  /* steps, alive_agents, alive_opps, escaping, escaping_time, episode  */
#define HH_TGT_K 3  /* stored sorted target list per unit (high level), ids / norm. distances; HighLevelEnv worlds with more than 3
                       aircraft on a side keep HH_TGT_K_WIDE entries (hh_spec.h: HH_TGT_K_OF) and their views are [N, A, 5] */
#define HH_TGT_K_WIDE 5
typedef struct hh_state_view {
    double *ac_f;   /* [N, A, HH_ACF_K] */
    int32_t *ac_i;  /* [N, A, HH_ACI_K] */
    double *rk_f;   /* [N, A, HH_RKF_K]  rocket slot s belongs to launcher slot s */
    int32_t *rk_i;  /* [N, A, HH_RKI_K] */
    int32_t *ar_i;  /* [N, HH_ARI_K] */
    int32_t *tgt_id; /* [N, A, K]  (0 = none), K = HH_TGT_K_OF(n_agents, n_opps) */
    double *tgt_d;   /* [N, A, K] */
} hh_state_view;

#define HH_SEL_OPP_SIDE 64 /* selector bit of an opponent's fight row when hh_config.opp_side_selector is set */

typedef struct hh_world hh_world;

/* ctor of LowLevelEnv / HighLevelEnv (env_hetero.py:20-51, env_hier.py:31-42) for N arenas */
int hh_world_create(const hh_config *cfg, int device, hh_world **out);
int hh_world_destroy(hh_world *w);
const char *hh_last_error(void);

/* observation width D (floats per controlled agent, zero padded): 26 fight / 30 escape / 34 commander */
int hh_obs_dim(const hh_world *w);
/* number of units whose actions the caller supplies per step: n_agents, or n_agents+n_opps
 * when ext_opp_actions */
int hh_n_ctrl(const hh_world *w);

/* reset() (env_base.py:62-77 + _reset_scenario 551-585 + state()): re-samples the arenas whose
 * mask byte is non-zero (mask [dev] u8[N]; NULL = all), episode += 1, and refreshes the
 * observation of those arenas into obs [dev] f32[N, n_agents, D] (may be NULL). */
int hh_reset(hh_world *w, const uint8_t *mask, float *obs, void *stream);

/* step() (env_base.py:79-109 -> env_hetero.py:105-186 _take_action -> cmano_simulator.py:138-157
 * do_tick -> env_hetero.py:188-225 rewards -> env_hetero.py:65-103 state).
 *   actions      [dev] i8 [N, n_ctrl, 4]   MultiDiscrete([13,9,2,2]); 4th ignored for type 2.  Components outside their ranges (the
 *                                          reference's spaces never emit them, env_hetero.py:37-43; its guards would raise, ac1.py:58-66)
 *                                          are SANITISED where the word is loaded — heading component clamped to [0, 12], speed component
 *                                          to [0, 8], fire components read as non-zero = fire (hh_spec.h: hh_action_sanitize) — and the
 *                                          arena's sticky fault flag is set (hh_action_faults).  Only CONSUMED words count: rows of dead
 *                                          units and of finished arenas may hold anything
 *   obs          [dev] f32[N, n_agents, D] observation after the tick (all agents, zeros if dead)
 *   reward       [dev] f32[N, n_agents]
 *   reward_valid [dev] u8 [N, n_agents]    1 iff the reference's rewards dict has the key
 *   done         [dev] u8 [N]              terminateds["__all__"]
 * Arenas already done (and not auto-reset) are left untouched and report reward_valid = 0. */
int hh_step(hh_world *w, const int8_t *actions, float *obs, float *reward, uint8_t *reward_valid,
            uint8_t *done, void *stream);

/* T consecutive steps from a pre-resident action tape in ONE launch sequence with no host
 * round trip: actions [dev] i8[T, N, n_ctrl, 4]; outputs are [T, ...] stacked like hh_step. */
int hh_rollout(hh_world *w, int32_t n_steps, const int8_t *actions, float *obs, float *reward,
               uint8_t *reward_valid, uint8_t *done, void *stream);

/* Levels 4-5 (ext_opp_actions): the opponents fly frozen policies that the reference evaluates INSIDE step(),
 * in unit id order after the agents acted (env_hetero.py:160-172, env_base.py:349-398).  Faithful split:
 *   hh_step_begin(agent_actions [dev] i8[N, n_agents, 4], opp_mode 0 fight / 1 escape)
 *       -> opp_obs [dev] f32[N, n_opps, 30]: lowlevel_state(opp_mode, i) of each live opponent (zeros if dead)
 *   (caller runs its frozen policies)
 *   hh_step_finish(opp_actions [dev] i8[N, n_opps, 4]) -> outputs exactly like hh_step.
 * hh_step with n_ctrl = n_agents + n_opps remains for callers that do not need the opponents' observations.
 * opp_mode = HH_OPP_MODE_EPISODE: level 5 in fight mode draws, per arena and per episode, which frozen policy set the
 * opponents fly (k = randint(3,5), env_hetero.py:55-59) and k == 5 means "escape": each arena then observes in the mode of
 * its own draw; hh_opp_policy reports k so that the caller evaluates policies[k]. */
#define HH_OPP_MODE_EPISODE (-1)
int hh_step_begin(hh_world *w, const int8_t *agent_actions, int32_t opp_mode, float *opp_obs, void *stream);
int hh_step_finish(hh_world *w, const int8_t *opp_actions, float *obs, float *reward, uint8_t *reward_valid,
                   uint8_t *done, void *stream);

/* level 5 / fight mode: k in {3,4,5} of every arena's CURRENT episode -> [dev] i8[N] (0 for every other configuration) */
int hh_opp_policy(hh_world *w, int8_t *k_out, void *stream);

/* current observation of every arena without stepping (state(): env_hetero.py:62-63 / env_hier.py:49-98) */
int hh_observe(hh_world *w, float *obs, void *stream);

/* HighLevelEnv.step (envs/env_hier.py:114-140) for 3-vs-3 worlds.  One commander step =
 *   hh_hl_begin(commander actions)            _action_assess + opponents' draws (142-190)
 *   up to 16 x { pilots(agents) -> hh_hl_agents_act -> pilots(opponents) -> hh_hl_tick }
 *   hh_hl_end                                 done, rewards, commander observation (49-98)
 * The frozen pilot policies (env_base.py:349-398) run in the caller between the launches on the
 * observations these calls emit: pilot_obs [dev] f32 [N, 6, 30] = lowlevel_state (env_hier.py:100-112)
 * of the side that acts next (agents after begin/tick, opponents after agents_act), zero elsewhere;
 * pilot_mode [dev] u8 [N, 6]: 0 = no action needed, else (policy type: 1 fight / 2 escape) | (aircraft type 1 / 2) << 2, i.e.
 * 5 = Fight1, 6 = Esc1, 9 = Fight2, 10 = Esc2 — the selector byte hh_policy_act (hh_policy.h) maps to a network.
 * actions [dev] i8 [N, 6, 4] (rows of the side that acts).  commander_actions [dev] i8 [N, 3] in {0,1,2}.
 * `running` (host, nullable): number of arenas still inside their macro step after this tick. */
int hh_hl_begin(hh_world *w, const int8_t *commander_actions, float *pilot_obs, uint8_t *pilot_mode, void *stream);
int hh_hl_agents_act(hh_world *w, const int8_t *actions, float *pilot_obs, uint8_t *pilot_mode, void *stream);
int hh_hl_tick(hh_world *w, const int8_t *actions, float *pilot_obs, uint8_t *pilot_mode, int32_t *running, void *stream);
int hh_hl_end(hh_world *w, float *obs, float *reward, uint8_t *reward_valid, uint8_t *done, void *stream);

/* The same commander step with ONE launch and ONE policy call per sub-step (worlds of up to 3 aircraft per side):
 *   hh_hl_begin_variants(commander actions) -> up to 16 x { pilots(all rows) -> hh_hl_act_tick } -> hh_hl_end
 * The standard path needs a launch per SIDE because the opponents' pilots observe the agents' weapon flags of the same sub-step (env_base.py:208-211,
 * units act in id order).  An agent's action can only RAISE its flag, and an opponent's row carries the flag of at most two agents, so these calls emit
 * each opponent's row together with its VARIANTS — the copies with the observed agents' still-zero flags forced to one — and hh_hl_act_tick, after
 * letting the agents act, takes each opponent's action from the variant that matches what happened.  Same rows through the same networks: the same
 * trajectories as the standard path, bit for bit — WHEN both run the same forward form of the policy kernel (a row's logits do not depend on its
 * tile, but the tile forms and the weights-through-LDS forms differ in the last bits, and the two paths' call sizes can fall on different sides of
 * the form threshold: a near-tie arg-max could then differ; pin the form with HH_POLICY_W / hh_policy_set_tile_rows for a bit-for-bit A/B).  Row slots per arena: HH_HL_VROWS = 15 = agents 0..2, then opponent j's variant v at 3 + 4 j + v
 * (v bit 0 / bit 1 = the first / second observed agent's flag forced; v = 0 is the row as the world stands).
 * pilot_obs [dev] f32 [N, 15, 30], pilot_mode [dev] u8 [N, 15] (0 = slot not in use), actions [dev] i8 [N, 15, 4] (the policy's output for every listed row).
 * A bound policy bank (hh_bind_policy) needs max_rows >= 15 * N. */
#define HH_HL_VROWS 15
int hh_hl_begin_variants(hh_world *w, const int8_t *commander_actions, float *pilot_obs, uint8_t *pilot_mode, void *stream);
int hh_hl_act_tick(hh_world *w, const int8_t *actions, float *pilot_obs, uint8_t *pilot_mode, int32_t *running, void *stream);

/* HighLevelEnv.step in ONE launch for callers whose pilot actions exist before the step starts (a recorded / scripted tape,
 * env-only throughput runs): pilot_tape [dev] i8 [16, N, 6, 4] = the actions of sub-step k in slice k (each side's rows are
 * read at its turn).  Same result as hh_hl_begin + 16 x {hh_hl_agents_act, hh_hl_tick} + hh_hl_end with those actions, bit
 * for bit; state stays in registers across the sub-steps and a workgroup stops as soon as none of its arenas is still inside
 * its macro step.  Pilot observations are not emitted (nobody reads them when the actions are already known). */
int hh_hl_rollout(hh_world *w, const int8_t *commander_actions, const int8_t *pilot_tape, float *obs, float *reward,
                  uint8_t *reward_valid, uint8_t *done, void *stream);

/* commander_actions of the current macro step after _action_assess (env_hier.py:142-190): agents' validated
 * actions and the opponents' drawn ones, [host] i8 [N, 6]; read by the eval_info counters (env_base.py:91-107) */
int hh_hl_commands(hh_world *w, int8_t *out);

/* cumulative arena-ticks run by HighLevelEnv macro steps on this world ([host] u64; synchronises `stream`): arenas leave
 * a macro step early (kill / surrounding event, env_hier.py:125), so ticks/s must be counted, not assumed 16 per step */
int hh_hl_tick_count(hh_world *w, uint64_t *out, void *stream);

/* name of the kernel instance hh_rollout / hh_step (or the hh_hl_* phases) launch for this world on this device */
int hh_rollout_kernel_name(hh_world *w, char *buf, int32_t len);

/* the same instance as a profiler prints it (demangled template arguments, e.g. "hh_k_world_quad<1, 1, true, 8>"): bench.py only
 * quotes counter evidence (profiles/latest_*.json) whose kernel name contains this string.  which = 0: the kernel of hh_rollout /
 * hh_step (LowLevelEnv) or of the hh_hl_* phase launches (HighLevelEnv); 1: the kernel of hh_hl_rollout */
int hh_kernel_instance(hh_world *w, int32_t which, char *buf, int32_t len);

/* Evaluation counters of HighLevelEnv.step (envs/env_base.py:91-107, read by evaluation.py:66-82), computed on the device
 * for every arena inside hh_hl_end: columns = agents_win, opps_win, draw (flags of the step that ended the episode),
 * agent_fight, agent_escape, opp_fight, opp_escape, agent_steps, opp_steps, opp1, opp2, opp3 (units that still exist after
 * the step, by their assessed commander action; oppK = agents fighting their K-th stored target).
 *   last  [dev] i32 [N, HH_EVAL_K]  nullable: the info dict of the most recent commander step of every arena
 *   total [dev] i32 [N, HH_EVAL_K]  nullable: summed over every commander step since the world was created / last cleared
 * clear_total != 0 zeroes the sums after copying them. */
#define HH_EVAL_K 12
int hh_eval_info(hh_world *w, int32_t *last, int32_t *total, int32_t clear_total, void *stream);

/* steps, alive_agents, alive_opps, done of every arena -> [dev] i32 [N, 4] (what step({}) needs: env_base.py:87-90) */
int hh_arena_status(hh_world *w, int32_t *out, void *stream);

/* Synthetic action tape of the benchmark workloads (BASELINE configs[1] "random actions": i.i.d. uniform over
 * MultiDiscrete([13,9,2,2]) from the keyed RNG, key = (seed, global arena, step, agent)): fills out [dev] i8 [T, N, n_units, 4]: the word at (t, n, s) is
 * hh_rng.h's `hh_rng_action_word` of seed, global arena arena_offset + n, step step0 + t, unit s + 1.  No world needed: the tape of a shard is the
 * slice of the global tape its arena_offset selects.  n_units = 2 for LowLevelEnv agents, 6 for a HighLevelEnv pilot tape. */
int hh_action_tape_uniform(uint64_t seed, uint64_t arena_offset, int32_t step0, int32_t T, int32_t N, int32_t n_units, int8_t *out, void *stream);

/* The device-side replacement of the reference's raising guards (ac1.py:58-66 set_heading / set_speed; SURVEY.md section 5 "invalid-state
 * flag per arena instead of raising"): out [dev] u8 [N] (nullable) = 1 for every arena in which, since the flags were last cleared, a step
 * (hh_step / hh_rollout / hh_step_begin / hh_step_finish / hh_hl_agents_act / hh_hl_tick / hh_hl_act_tick / hh_hl_rollout) consumed an action word with a
 * component outside MultiDiscrete([13,9,2,2]); that step ran on the sanitised word (see hh_step).  clear != 0 zeroes the flags after
 * copying them.  Resets do not clear them.  Ordered on `stream`, no host synchronisation. */
int hh_action_faults(hh_world *w, uint8_t *out, int32_t clear, void *stream);

/* Trajectory ring buffer on the device (rendering / trace export; cmano_simulator.py:125-130,159-162 record_unit_trace,
 * env_base.py:587-645 plot): after hh_trace_enable the first n_arenas arenas append one row per unit after every reset and every
 * tick, HH_TRACE_F floats = lat, lon, heading, speed, alive, rocket lat, rocket lon, rocket alive + 16 * episode; the ring keeps
 * the last `capacity` rows.  hh_trace_read copies it out: rows [host] f32 [capacity, n_arenas, A, HH_TRACE_F] (slot = row index
 * % capacity), count [host] i32 [n_arenas] = rows written so far.  While tracing is on, 2-vs-2 rollouts run on the generic kernel. */
#define HH_TRACE_F 8
int hh_trace_enable(hh_world *w, int32_t n_arenas, int32_t capacity);
int hh_trace_read(hh_world *w, float *rows, int32_t *count);

/* per-arena statistics of the most recently FINISHED episode (logging; this is what the
 * multi-GPU all-gather moves): ret [dev] f32[N] (sum of agent rewards), len [dev] i32[N],
 * outcome [dev] i8[N] (1 agents win, -1 opponents win, 0 draw, 2 none finished yet) */
int hh_episode_stats(hh_world *w, float *ret, int32_t *len, int8_t *outcome, void *stream);
/* the same three statistics as one [dev] f32[N, 3] block (return, length, outcome as floats), written by one small
 * launch: the block each rank contributes to the logging all-gather (hhmarl_2d_amd/sharding.py) */
int hh_episode_stats_packed(hh_world *w, float *out, void *stream);

/* Generalised advantage estimation on the stacked outputs of hh_rollout (what RLlib's postprocessing does
 * for the reference: train_hetero.py:216 gamma=0.99, lambda_=0.95, complete episodes).  All [dev]:
 * reward, valid, adv, ret [T, N, n_agents]; value [T+1, N, n_agents] (critic incl. bootstrap row); done [T, N].
 * Not tied to a world: launches on the calling thread's current device, which must own the buffers. */
int hh_gae(int32_t T, int32_t N, int32_t n_agents, const float *reward, const float *value, const uint8_t *valid,
           const uint8_t *done, float gamma, float lam, float *adv, float *ret, void *stream);

/* The same scan with the semantics RLlib 2.4 gives the reference's step stream (what train_hetero.py / train_hier.py actually
 * train on): no reward key = reward 0.0 and the row stays in the trajectory (the reference returns observations for dead agents,
 * env_hetero.py:65-103,217-223, and RLlib's sampler reads rewards[env_id].get(agent_id, 0.0)); last_r = 0.0 after every episode
 * end; delta and the discounted sum in float64 (np.concatenate with last_r promotes, scipy.signal.lfilter inside discount_cumsum
 * (ray/rllib/evaluation/postprocessing.py).  `reward` must hold 0.0 where hh_rollout reported reward_valid = 0 (it does).
 * train_hetero.py:216: gamma 0.99, lambda 0.95; train_hier.py:186: gamma 0.99 and RLlib's default lambda 1.0. */
int hh_gae_rllib(int32_t T, int32_t N, int32_t n_agents, const float *reward, const float *value, const uint8_t *done, double gamma,
                 double lam, float *adv, float *ret, void *stream);

/* Whole-episode batches (batch_mode = "complete_episodes", train_hetero.py:212 / train_hier.py:182): RLlib gives its learner only
 * whole episodes, from the reset row to the done row, with GAE over each episode and last_r = 0 at its end.  hh_episodes_emit takes
 * one collect's [T, N, ...] buffers (auto-resetting arenas: the row after a done is the next episode's reset row), keeps every arena's
 * running episode in a device-side carry across calls, and writes the rows of every episode that ended in this window — the carried
 * rows first, then the window's — into one flat batch, arena-major, then episode, then time (fixed by a scan, not by scheduling).
 * advantages / value targets are hh_gae_rllib's recursion (float64 delta and discounted sum, float32 results) run over each whole
 * episode with last_r = 0.0.  Not tied to a world: generic in n_agents and the observation width; launches on the calling thread's
 * current device, which must own every buffer; no host synchronisation and no allocation (graph-capturable).  All pointers [dev].
 * Capacities: an episode has at most `horizon` rows, so carry_cap = horizon - 1 rows per arena and row_cap = N (carry_cap + T) rows
 * per call never overflow, ep_cap = N T episodes per call; if they did anyway, counts[2] is set (sticky) and nothing is written out of
 * bounds.  The caller zeroes carried / episode (and counts) before the first call and whenever its arenas are reset. */
typedef struct hh_episode_bufs {
    int32_t T;                /* ticks per call */
    int32_t N;                /* arenas */
    int32_t n_agents;         /* agents per arena row */
    int32_t obs_dim;          /* D: floats per agent in an observation row */
    int32_t carry_cap;        /* rows per arena the carry holds (horizon - 1) */
    int32_t reserved0;        /* must be 0 */
    int64_t row_cap;          /* rows of every output column (N (carry_cap + T); < 2^31) */
    int64_t ep_cap;           /* entries of the episode table (N T) */
    double gamma;
    double lam;
    /* one collect (read): obs f32 [T(+1), N, n_agents, D], actions i8 [T, N, n_agents, 4], logp / vf (T(+1)) / reward f32 [T, N, n_agents],
       valid u8 [T, N, n_agents], done u8 [T, N] */
    const float *obs;
    const int8_t *actions;
    const float *logp;
    const float *vf;
    const float *reward;
    const uint8_t *valid;
    const uint8_t *done;
    /* carry (read and written): the same columns [N, carry_cap, ...] */
    float *c_obs;
    int8_t *c_actions;
    float *c_logp;
    float *c_vf;
    float *c_reward;
    uint8_t *c_valid;
    int32_t *carried;         /* [N] rows held per arena */
    int32_t *episode;         /* [N] episodes finished per arena (the `episode` column of the next one) */
    int32_t *scratch;         /* [5, N] */
    /* batch (written): the collect's columns [row_cap, ...], then adv / target f32 [row_cap, n_agents], done u8 [row_cap] (1 on an
       episode's last row only), arena / episode / t i32 [row_cap] (t = step within the episode, from 0) */
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
    int32_t *ep_start;        /* [ep_cap] first row of each episode in the batch */
    int32_t *ep_len;          /* [ep_cap] */
    int32_t *ep_arena;        /* [ep_cap] */
    int32_t *counts;          /* [3]: rows, episodes written by this call; overflow flag (sticky) */
} hh_episode_bufs;

int hh_episodes_emit(const hh_episode_bufs *b, void *stream);

/* One optional per-agent float column that travels with the rows of a whole-episode batch (hh_episodes_emit_aux, and
 * hh_commander_episodes_emit_aux of hh_commander.h): aux_dim floats per agent and row, moved in the same pass and into the same row
 * order as obs — through the carry, into the batch, bit for bit.  The emitter does not interpret it (the rollouts put the sampler's
 * logits there: RLlib's ACTION_DIST_INPUTS).  4-byte alignment suffices; where a row of n_agents aux_dim floats is a multiple of 16
 * bytes and all three bases are 16-byte aligned the column moves in 16-byte units.  All pointers [dev]. */
#define HH_EP_AUX_MAX_DIM 32
typedef struct hh_episode_aux {
    int32_t aux_dim;          /* floats per agent: 1 .. HH_EP_AUX_MAX_DIM */
    int32_t reserved0;        /* must be 0 */
    const float *aux;         /* one collect (read): [T, N, n_agents, aux_dim] */
    float *c_aux;             /* carry (read and written): [N, carry_cap, n_agents, aux_dim] */
    float *o_aux;             /* batch (written): [row_cap, n_agents, aux_dim] */
} hh_episode_aux;

/* hh_episodes_emit with the aux column; x = NULL: hh_episodes_emit exactly.  The same launches, capacities and overflow flag (a row
 * that is not written is not written in any column); HH_E_ARG for aux_dim out of range, reserved0 != 0, a null or misaligned buffer. */
int hh_episodes_emit_aux(const hh_episode_bufs *b, const hh_episode_aux *x, void *stream);

/* Accumulated batches (RLlib's train_batch_size: training_step concatenates whole sample batches until at least that many environment
 * steps are there, trims nothing, then runs one update).  hh_episodes_emit_append is hh_episodes_emit_aux (x = NULL: no aux column)
 * that APPENDS to the batch in place: the same four launches, no host synchronisation, no allocation, graph-capturable.  Its scan
 * starts from the device-side accumulator `acc` instead of 0:
 *   - acc[4] set (the previous call completed a batch): this call starts the next one — base rows, episodes and sequences are 0,
 *     acc[5] restarts at 0 and acc[6] goes up by one; otherwise the bases are acc[0], acc[1], acc[3];
 *   - every arena's row, episode and sequence offset is base + its exclusive scan, so ep_start (and the commander's seq_start / seq_ep)
 *     are absolute positions in the accumulated batch; the order is collect-major, then arena, episode, time;
 *   - afterwards acc[0], acc[1], acc[3] = base + this call's totals (clamped to the capacities), acc[4] = acc[0] >= train_rows,
 *     acc[5] += 1; acc[2] (sticky, like counts[2], which is set with it) is set if base + totals exceeds a capacity or counts[2] was
 *     already set; counts[0], counts[1], counts[3] keep meaning "written by this call";
 *   - GAE runs over the episodes this call appended only, [acc[1] - counts[1], acc[1]): adv / target of earlier episodes are not
 *     rewritten;
 *   - totals (NULL, or [dev] i64 [2], 8-byte aligned): totals[0] += counts[1], totals[1] += counts[0] — every episode and row once.
 * row_cap / ep_cap (/ seq_cap) are the capacities of the ACCUMULATED batch: a batch was below train_rows before its last call, so
 * row_cap = train_rows - 1 + N (carry_cap + T), ep_cap = train_rows - 1 + N T never overflow.  With train_rows = 1 and a zeroed acc
 * every call writes exactly the bytes of hh_episodes_emit_aux (a batch with any row is complete: the next call starts at 0).  The
 * caller zeroes acc before the first call; zeroing it later discards a partial batch (the carry is untouched).
 * HH_E_ARG, nothing launched: train_rows < 1, acc NULL or not 4-byte aligned, totals not 8-byte aligned, and whatever
 * hh_episodes_emit_aux refuses. */
#define HH_EP_ACC 8   /* i32 [8] on the device: [0] rows, [1] episodes, [2] overflow (sticky), [3] sequences, [4] batch complete
                         (rows >= train_rows), [5] collects in this batch, [6] batches completed, [7] 0 */
int hh_episodes_emit_append(const hh_episode_bufs *b, const hh_episode_aux *x, int64_t train_rows, int32_t *acc, int64_t *totals,
                            void *stream);

/* Episode metrics of one emitted whole-episode batch (RLlib's per-iteration result: episode_reward_mean/min/max, episode_len_mean,
 * episodes_this_iter, policy_reward_*, vf_explained_var, episodes_total, timesteps_total), computed on the device right behind
 * hh_episodes_emit / hh_commander_episodes_emit from the batch's reward / vf / target columns and its episode table.  Three launches
 * on `stream`, no host synchronisation, no allocation (graph-capturable).  The numbers of rows and episodes are READ FROM `counts`
 * ON THE DEVICE (clamped to the capacities); rows and table entries beyond them are never read.
 *   ep_return[e, a]  the sum of reward[ep_start[e] .. ep_start[e] + ep_len[e] - 1, a] in float64 (NaN for a table entry that does not lie
 *                    inside the emitted rows: only after an emitter overflow, which counts[2] reports)
 *   summary          f64 [HH_EP_METRICS], the slots below.  An episode's reward is the sum of its agents' returns (in agent order), as
 *                    RLlib counts it; the per-agent slots [a] are RLlib's policy_reward_*, slots of agents >= n_agents are NaN.
 *                    explained variance of agent a = max(-1, 1 - Var(target - vf) / Var(target)) over ALL emitted rows of that agent
 *                    (ray/rllib/utils/torch_utils.py explained_variance; the two variances' common divisor cancels), from two-pass
 *                    sums of squared deviations (no E[x^2] - E[x]^2): per tile of 1024 rows around the tile's own mean, the tiles
 *                    combined around the global mean (sum M2_i + n_i (mean_i - mean)^2).
 *   totals           i64 [2], accumulated: [0] episodes_total += episodes, [1] timesteps_total += rows.  timesteps_total counts
 *                    ENVIRONMENT steps (one per emitted row, whatever n_agents), not agent steps.  The caller zeroes it.
 * With 0 episodes: episodes = rows = 0, every other slot NaN, totals unchanged.
 * Determinism: float64, no floating-point atomics; every sum has a fixed order that does not depend on the grid size (an episode: lane
 * l of its wave adds rows l, l + 64, ... in order, then a butterfly over the 64 lanes; the row tiles: likewise per workgroup, partials
 * into `scratch`; the last launch is one workgroup that folds episodes and tile partials in index order) — the same inputs give the
 * same bytes on every run.
 * HH_E_ARG, nothing enqueued: m = NULL, a NULL pointer, n_agents outside 1 .. HH_EP_METRICS_MAX_AGENTS, reserved0 != 0, row_cap
 * outside 1 .. 2^31 - 1024 (tiles of 1024 rows are counted in 32 bits) or ep_cap outside 1 .. 2^31 - 1, reward / vf / target / ep_start /
 * ep_len / counts not 4-byte aligned, ep_return / summary / totals / scratch not 8-byte aligned, scratch_bytes below
 * hh_episodes_metrics_scratch_bytes(ep_cap, row_cap, n_agents). */
#define HH_EP_METRICS_MAX_AGENTS 5
#define HH_EPM_EPISODES 0          /* episodes of this batch (episodes_this_iter) */
#define HH_EPM_ROWS 1              /* rows of this batch (environment steps) */
#define HH_EPM_REWARD_MEAN 2       /* episode reward: mean, min, max over the batch's episodes */
#define HH_EPM_REWARD_MIN 3
#define HH_EPM_REWARD_MAX 4
#define HH_EPM_LEN_MEAN 5          /* episode length in rows: mean, min, max */
#define HH_EPM_LEN_MIN 6
#define HH_EPM_LEN_MAX 7
#define HH_EPM_AGENT_MEAN 8        /* [5] per agent: return mean, min, max over the batch's episodes */
#define HH_EPM_AGENT_MIN 13
#define HH_EPM_AGENT_MAX 18
#define HH_EPM_AGENT_EXPLAINED_VAR 23 /* [5] per agent: vf_explained_var over the batch's rows */
#define HH_EP_METRICS 28           /* length of the summary block */
typedef struct hh_episode_metrics_bufs {
    int32_t n_agents;         /* 1 .. HH_EP_METRICS_MAX_AGENTS */
    int32_t reserved0;        /* must be 0 */
    int64_t row_cap;          /* rows of the batch's columns */
    int64_t ep_cap;           /* entries of the episode table */
    const float *reward;      /* [dev] f32 [row_cap, n_agents]: the emitted batch's columns (o_reward, o_vf, o_target) */
    const float *vf;
    const float *target;
    const int32_t *ep_start;  /* [dev] i32 [ep_cap] */
    const int32_t *ep_len;    /* [dev] i32 [ep_cap] */
    const int32_t *counts;    /* [dev] the emitter's counts: [0] rows, [1] episodes, [2] overflow flag */
    double *ep_return;        /* [dev] f64 [ep_cap, n_agents] out */
    double *summary;          /* [dev] f64 [HH_EP_METRICS] out */
    int64_t *totals;          /* [dev] i64 [2] in/out: episodes_total, timesteps_total (accumulated) */
    void *scratch;            /* [dev] scratch_bytes >= hh_episodes_metrics_scratch_bytes(...), 8-byte aligned */
    int64_t scratch_bytes;
} hh_episode_metrics_bufs;

int hh_episodes_metrics_scratch_bytes(int64_t ep_cap, int64_t row_cap, int32_t n_agents, int64_t *bytes);
int hh_episodes_metrics(const hh_episode_metrics_bufs *m, void *stream);

/* The same metrics for FIXED-WINDOW rollouts (batch_mode = "truncate_episodes"), computed on the device right behind the window's
 * hh_gae_rllib.  A window of T steps cuts episodes, so every arena carries its running episode's return and length across calls, and
 * the episodes that finish inside a window are tabulated and summarised.  Five launches on `stream`, no host synchronisation, no
 * allocation (graph-capturable), no atomics of any kind.  For arena n, t = 0 .. T-1 in order:
 *   run_return[n, a] += (double)reward[t, n, a]   ONE float64 addition per row, in time order, across windows: a host restatement with
 *                                                 sequential sums gives the same bits, wherever the windows cut the episode
 *   run_len[n] += 1
 *   where done[t, n] != 0: the next table entry gets ep_arena = n, ep_end = t, ep_len = run_len[n], ep_return = run_return[n, :] — the
 *                          rows of earlier windows included — and both running values go back to 0.
 * The table is arena-major, then t; it has at most T N entries, so nothing can overflow; entries beyond counts[0] are never written.
 *   counts           i32 [2] out: [0] episodes that ended in this window, [1] rows = T N
 *   summary          f64 [HH_EP_METRICS]: the HH_EPM_* slots with exactly hh_episodes_metrics' meaning — an episode's reward is the sum
 *                    of its agents' returns in agent order, the per-agent mean / min / max are over the window's finished episodes,
 *                    the explained variance of agent a is over ALL T N rows of the window (target against rows 0 .. T-1 of vf), by the
 *                    same two-pass tile scheme; rows = T N in every call.
 *   totals           i64 [2], accumulated: [0] episodes_total += episodes, [1] timesteps_total += T N (environment steps).  The caller
 *                    zeroes it, and run_return / run_len, before the first window.
 * ONE DIFFERENCE from hh_episodes_metrics, on purpose: with 0 episodes, episodes = 0, rows = T N and the explained variances are still
 * computed; only the episode slots (reward, length, per-agent mean / min / max) are NaN, and totals[1] += T N all the same — a window's
 * steps count whether or not an episode ended in it.
 * Determinism: float64; the carry is one sequential chain per arena and agent; the table's order comes from an exclusive scan of the
 * arenas' counts; the summary's sums are hh_episodes_metrics' (fixed order, independent of the grid size) — the same inputs give the
 * same bytes on every run.
 * HH_E_ARG, nothing enqueued (hh_last_error() starts with "hh_window_metrics: "): m = NULL, a NULL pointer, T < 1, N < 1, T N above
 * 2^31 - 1024, n_agents outside 1 .. HH_EP_METRICS_MAX_AGENTS, reserved0 != 0, reward / vf / target / run_len / ep_len / ep_arena /
 * ep_end / counts not 4-byte aligned, run_return / ep_return / summary / totals / scratch not 8-byte aligned, scratch_bytes below
 * hh_window_metrics_scratch_bytes(T, N, n_agents). */
typedef struct hh_window_metrics_bufs {   /* field order is ABI; host struct of device pointers */
    int32_t T, N, n_agents, reserved0;    /* n_agents 1 .. HH_EP_METRICS_MAX_AGENTS; reserved0 must be 0 */
    const float *reward;                  /* [dev] f32 [T, N, n_agents]  the window as the rollouts hold it */
    const float *vf;                      /* [dev] f32 [T+1, N, n_agents]; rows 0 .. T-1 are read */
    const float *target;                  /* [dev] f32 [T, N, n_agents] */
    const uint8_t *done;                  /* [dev] u8  [T, N] */
    double *run_return;                   /* [dev] f64 [N, n_agents] in/out: return so far of every arena's running episode */
    int32_t *run_len;                     /* [dev] i32 [N] in/out: its rows so far */
    double *ep_return;                    /* [dev] f64 [T N, n_agents] out: episodes that ended in this window */
    int32_t *ep_len, *ep_arena, *ep_end;  /* [dev] i32 [T N] out: rows of the whole episode, its arena, the t of its done row */
    int32_t *counts;                      /* [dev] i32 [2] out: episodes, rows (= T N) */
    double *summary;                      /* [dev] f64 [HH_EP_METRICS] out: the HH_EPM_* slots, unchanged */
    int64_t *totals;                      /* [dev] i64 [2] in/out: episodes_total, timesteps_total */
    void *scratch; int64_t scratch_bytes;
} hh_window_metrics_bufs;
int hh_window_metrics_scratch_bytes(int32_t T, int32_t N, int32_t n_agents, int64_t *bytes);
int hh_window_metrics(const hh_window_metrics_bufs *m, void *stream);

/* Win / lose / draw of every training episode.  The step kernels write an arena's outcome (hh_episode_stats' codes) when it finishes an
 * episode, and under auto-reset its next finished episode overwrites the value.  hh_outcome_tap, enqueued right behind a tick, keeps it:
 *   out_row[n] = done_row[n] != 0 ? last_outcome[n] : HH_OUTCOME_NONE          for all N arenas of the world
 * done_row [dev] u8 [N] is the tick's done output, out_row [dev] i8 [N].  One small launch on `stream`; it only reads the world, makes
 * no allocation and no synchronisation (graph-capturable).  HH_E_ARG (hh_last_error() starts with "hh_outcome_tap: ") for a NULL
 * argument. */
#define HH_OUTCOME_WIN 1       /* agents win */
#define HH_OUTCOME_LOSE (-1)   /* opponents win */
#define HH_OUTCOME_DRAW 0
#define HH_OUTCOME_NONE 2      /* no episode finished (hh_episode_stats: none finished yet) */
int hh_outcome_tap(hh_world *w, const uint8_t *done_row, int8_t *out_row, void *stream);

/* The outcomes of an episode table and their summary, behind hh_episodes_emit* / hh_commander_episodes_emit* (+ hh_episodes_metrics) or
 * hh_window_metrics.  Both tables list the episodes that ended in a window arena-major, then in time, so the j-th done row of arena n is
 * the window's entry e0 + offset(n) + j: offset is the exclusive scan of the arenas' done counts, m their total, and e0 = e1 - m with e1
 * the table's device count (the window's segment is the table's last one — also in a batch that accumulates under
 * hh_episodes_emit_append).  Two launches on `stream` (count, then one workgroup: scan, check, write, summary), no host synchronisation,
 * no allocation (graph-capturable), no atomics; nothing but the outputs below is written.
 *   ep_outcome       i8 [ep_cap]: entry e0 + offset(n) + j = outcome[t, n] at arena n's j-th done row t.  Only [e0, e1) is written:
 *                    earlier segments keep their bytes.
 *   summary          f64 [HH_EO_SUMMARY] over the entries [0, e1): [0] episodes (e1); [1..3] episodes won / lost / drawn (codes 1 / -1 /
 *                    0); [4..6] the mean episode reward per class, an episode's reward being the sum of its agents' ep_return in agent
 *                    order (hh_episodes_metrics' convention); [7..9] the mean ep_len per class; [10] entries with any other code;
 *                    [11] 0.  A class without an episode has count 0 and NaN means.
 *   flags            i32 [2]: [0] != 0 when e1 < m or some ep_arena[e0 + offset(n) + j] != n — the table does not hold this window's
 *                    episodes (after an emitter overflow, say) — and then NOTHING is written to ep_outcome; [1] = m.
 * e1 is read on the device from n_episodes[0] and clamped to 0 .. ep_cap.
 * Determinism: float64; the order of the entries comes from the scan; the summary adds tiles of 1024 entries in index order, inside a
 * tile one entry per lane, a butterfly over each wave's 64 lanes and the 16 waves in index order — the same inputs give the same bytes
 * on every run.
 * HH_E_ARG, nothing enqueued (hh_last_error() starts with the function's name): b = NULL, a NULL pointer, T < 1, N < 1, T N above
 * 2^31 - 1024, ep_cap outside 1 .. 2^31 - 1024, n_agents outside 1 .. HH_EP_METRICS_MAX_AGENTS, reserved0 != 0, n_episodes / ep_arena /
 * ep_len / flags not 4-byte aligned, ep_return / summary / scratch not 8-byte aligned, scratch_bytes below
 * hh_episode_outcomes_scratch_bytes(T, N, ep_cap). */
#define HH_EO_SUMMARY 12
typedef struct hh_episode_outcome_bufs {   /* field order is ABI; host struct of device pointers */
    int32_t T, N, n_agents, reserved0;     /* n_agents 1 .. HH_EP_METRICS_MAX_AGENTS; reserved0 must be 0 */
    int64_t ep_cap;                        /* entries of the episode table */
    const uint8_t *done;                   /* [dev] u8 [T, N]  the window */
    const int8_t *outcome;                 /* [dev] i8 [T, N]  hh_outcome_tap's rows */
    const int32_t *n_episodes;             /* [dev] i32 [1]: e1, the table's count (the emitter's counts[1] / acc[1], hh_window_metrics' counts[0]) */
    const int32_t *ep_arena;               /* [dev] i32 [ep_cap] */
    const int32_t *ep_len;                 /* [dev] i32 [ep_cap] */
    const double *ep_return;               /* [dev] f64 [ep_cap, n_agents] */
    int8_t *ep_outcome;                    /* [dev] i8 [ep_cap] out */
    double *summary;                       /* [dev] f64 [HH_EO_SUMMARY] out */
    int32_t *flags;                        /* [dev] i32 [2] out */
    void *scratch; int64_t scratch_bytes;  /* [dev] >= hh_episode_outcomes_scratch_bytes(...), 8-byte aligned */
} hh_episode_outcome_bufs;
int hh_episode_outcomes_scratch_bytes(int32_t T, int32_t N, int64_t ep_cap, int64_t *bytes);
int hh_episode_outcomes(const hh_episode_outcome_bufs *b, void *stream);

/* Test probe: the shared math of include/hh_math.h / hh_geodesic.h evaluated ON THE DEVICE over arrays of operands, so that a
 * -m gpu test can compare the kernels' arithmetic with the CPU oracle's bit for bit (tests/test_gpu_math.py), not only through
 * trajectories.  fn: 0 sincos(a) -> o0, o1 | 1 atan2(a, b) | 2 acos(a) | 3 sincosd(a) -> o0, o1 | 4 atan2d(a, b) | 5 pymod(a, b) |
 * 6 remainder(a, b) | 7 fmod(a, b) | 8 round3(a) | 9 a / b by hh_div_known | 10 pymod_turn(a, b) | 11 sqrt(a) | 12 clip(a, 0, 1) |
 * 13 clip(a, -b, b) | 14 geo_move(lat = a, lon = b, azi = o0_in, s = o1_in) -> o0, o1 (the outputs carry the third and fourth
 * operand in).  a, b, o0, o1: device arrays of n doubles. */
int hh_math_eval(int32_t fn, int32_t n, const double *a, const double *b, double *o0, double *o1, void *stream);

/* host snapshot in / out (synchronises the stream) */
int hh_get_state(hh_world *w, hh_state_view *view);
int hh_set_state(hh_world *w, const hh_state_view *view);

/* integer event masks of the last step, for bit-exact parity checks ([host]; ordered after the work queued on
 * `stream` and synchronises that stream only):
 * per arena u32: bits 0..7 units killed by cannon, 8..15 killed by rocket, 16..23 out of bounds,
 * 24..31 missile launched this step (by unit slot); ten-slot arenas (more than 3 aircraft on a side): hh_spec.h HH_EV_BIT */
int hh_get_event_masks(hh_world *w, uint32_t *masks, void *stream);

/* Complete snapshots (checkpointing a RUNNING world; csrc/hh_snapshot.h).  hh_get_state / hh_set_state carry the simulation state only:
 * a world also keeps, across launches, the running episode return and the statistics of the last finished episode (hh_episode_stats), the
 * rewards accumulated inside a HighLevelEnv macro step and its eval_info counters (hh_eval_info), the sticky action-fault flags
 * (hh_action_faults), the commands and pilot modes of the macro step in flight, the level-5 per-episode policy draw's counters
 * (hh_opp_policy), the event masks, the macro-step counter words (hh_hl_tick_count) and, with a bound policy bank (hh_bind_policy), the
 * bank's row counters and row lists.  A snapshot holds all of it, as opaque bytes [host]:
 *     header (208 bytes): magic u32 "HHSW", format version u32 (1), digest u64 (FNV-1a of the creating hh_config), N i32, A i32,
 *                         slot count i32 (0), sections i32 (4), layout words i32 [12] ([0] = max_rows of the bound bank, 0 without
 *                         one), section sizes u64 [16]
 *     sections, each on a 16-byte boundary: 0 the creating hh_config | 1 the world's device arrays (one slab) | 2 the bound bank's
 *                         row counters | 3 its row lists (2, 3: empty without a bound bank)
 * The trajectory ring of hh_trace_enable is NOT saved: a restore leaves tracing (on or off, the ring's rows and cursors) as the
 * receiving world has it.  Kernel-instance choices (HH_FORCE_W and its like) belong to the receiving process too.
 *   hh_world_snapshot_bytes  *bytes = size of this world's snapshot
 *   hh_world_snapshot        host_buf [host] of at least that size <- the snapshot; ordered behind the work queued on `stream`
 *   hh_world_restore         the snapshot -> the world.  The WHOLE header is checked before anything is written: a blob of another
 *                            n_arenas, env kind, level, mode, seed, arena_offset (any other field of hh_config), another bound-bank
 *                            size, another format version, or a buffer shorter than the snapshot returns HH_E_ARG with the reason in
 *                            hh_last_error() and leaves the world untouched.
 * Copies only (no kernel is launched); snapshot and restore synchronise `stream`, like hh_get_state.  A restore into a freshly created
 * world of the same hh_config needs no hh_reset first. */
int hh_world_snapshot_bytes(hh_world *w, int64_t *bytes);
int hh_world_snapshot(hh_world *w, void *host_buf, int64_t bytes, void *stream);
int hh_world_restore(hh_world *w, const void *host_buf, int64_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HH_ABI_H */
