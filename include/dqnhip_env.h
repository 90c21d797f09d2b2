/*
 * dqnhip_env.h — batched environment front-end for the learner of dqnhip.h.
 *
 * Replaces, for N concurrent workers whose state vectors live in HBM, the per-agent episode
 * loop of the reference's src/dqn_main.cpp:97-153 (PlayOneEpisode) on the learner side:
 *     SelectAction(state, epsilon)            src/dqn.cpp:684-711  (one epsilon draw per call)
 *     GetAction(actor_output)                 src/dqn.cpp:196-208
 *     HFOGameState::update + reward           src/hfo_game.cpp:122-236
 *     Transition(state, actor_output, reward, 0, next | none)   src/dqn_main.cpp:138-141
 *     LabelTransitions + AddTransitions at episode end          src/dqn_main.cpp:145-150
 * The HFO server itself (rcssserver over UDP inside hfo.step()) is outside the reference repo
 * and absent here; the state stream it would deliver is replaced by a SYNTHETIC generator
 * (features U(-1,1), indices 12/54 in {-1,+1}, (13,14)/(51,52) = (sin,cos) of a
 * uniform angle, geometric episode length capped at --frames-per-trial) driven by the same
 * counter-based RNG on the device and in the CPU oracle, so the two can be compared
 * transition by transition.  Everything downstream of the state stream is the reference's
 * learner-side logic.
 *
 * A handle of the EXTERNAL kind (dqnhip_env_create_external) runs the same learner-side logic on
 * states the caller supplies — a rack of HFO servers, or any batched simulator that emits HFO
 * low-level features.  Its step is cut in two where the simulator sits: dqnhip_env_act is the step
 * up to GetAction, dqnhip_env_observe the rest.  Reward shaping, the episode buffers,
 * LabelTransitions and AddTransitions stay on the device; with DQNHIP_ENV_NO_RECORD it plays
 * PlayOneEpisode(update = false), the mode of Evaluate() (src/dqn_main.cpp:171-204).
 */
#ifndef DQNHIP_ENV_H_
#define DQNHIP_ENV_H_

#include <stdint.h>

#include "dqnhip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dqnhip_env_config {
  int32_t struct_size;   /* = sizeof(dqnhip_env_config) */
  int32_t workers;       /* concurrent HFO workers (agents) feeding this learner's replay */
  int32_t max_steps;     /* --frames-per-trial (500, src/hfo_game.cpp:8): forced OUT_OF_TIME */
  int32_t unum;          /* our uniform number (HFOGameState::our_unum) */
  float p_end;           /* per-step probability that the synthetic episode ends (1/mean length) */
  float p_goal;          /* given an end, probability that the status is GOAL */
  uint64_t seed;         /* key of the counter-based generator */
} dqnhip_env_config;

typedef struct dqnhip_env* dqnhip_env_handle;

/* Creates N workers attached to learner `h` (their transitions go to its replay ring) and
 * resets every worker: first synthetic state, HFOGameState() + the initial update that
 * PlayOneEpisode performs after its forced DASH(0,0) (src/dqn_main.cpp:103-105). */
int dqnhip_env_create(dqnhip_handle h, const dqnhip_env_config* cfg, dqnhip_env_handle* out);
int dqnhip_env_destroy(dqnhip_env_handle e);

/* Synthetic handles only (an external handle is stepped by dqnhip_env_act / dqnhip_env_observe).
 * Advance every worker by n_steps environment steps (N * n_steps transitions).  Per step:
 * one batched actor forward over the N current states, per-worker epsilon draw (random
 * ActorOutput with GetRandomActorOutput's ranges, src/dqn.cpp:664-682, or the greedy
 * output), GetAction, synthetic next state + status, HFOGameState update + reward,
 * transition appended to the worker's episode; finished episodes are labelled
 * (LabelTransitions) and appended to the replay ring in worker order (AddTransitions).
 * Asynchronous on the learner's stream. */
int dqnhip_env_step(dqnhip_env_handle e, float epsilon, int32_t n_steps);

/* Blocks; totals since creation: transitions generated, episodes finished, sum of rewards,
 * goals.  Also refreshes the learner's host-side memory_size.  Both kinds of handle. */
int dqnhip_env_stats(dqnhip_env_handle e, int64_t* env_steps, int64_t* episodes, double* reward_sum,
                     int64_t* goals);

/* Parity / debugging: per-worker values of the LAST step.  name: "action" [N] (GetAction index),
 * "arg1" [N], "arg2" [N], "reward" [N], "actor_out" [N,10], "state" [N,S] (current state),
 * "episode_len" [N]; "truncated" [1] (episodes an external handle closed at max_steps); "graph_nodes" [2] (launches in the
 * captured one-step and 16-step graphs of a synthetic handle, 0 while not captured). */
int dqnhip_env_debug_read(dqnhip_env_handle e, const char* name, float* host, size_t count);

/* Exploration noise on the greedy ActorOutput, both kinds of handle (semantics, key and defaults: "action noise" in dqnhip.h).
 * cfg NULL switches it off.  Off is the state at creation, and a handle that stays there launches what it always launched.
 * With noise on, every step draws ten normals per worker and advances the worker's OU state (on an epsilon-random step too, whose
 * random row stays un-noised); on a greedy step the noisy row is what opens the transition (the episode row, and through it the
 * replay memory), what dqnhip_env_act hands out as actor_out, and what GetAction reads.  The state is zero after a step that ends
 * the worker's episode.  It works in both acting precisions: the noise sits behind the heads.  cfg->clip is not used.
 * Every call zeroes all OU states and drops the handle's captured steps (the config is a kernel argument), blocking once.
 * dqnhip_env_debug_read then also knows "greedy_out" [N,10] (the heads' own output), "noise_state" [N,10] (the OU states after the
 * last step) and "noise_z" [N,10] (the last step's draws), and its "actor_out" is the row the last step chose (noisy greedy or
 * random; before the first step with noise: the greedy row). */
int dqnhip_env_set_noise(dqnhip_env_handle e, const dqnhip_noise_config* cfg);

/* ---- the external kind: states from the caller ------------------------------------------------ */

#define DQNHIP_ENV_NO_RECORD 1   /* PlayOneEpisode(update = false): nothing reaches the replay memory */

/* One finished episode: what PlayOneEpisode returns (src/dqn_main.cpp:151-152). */
typedef struct dqnhip_env_episode {
  double total_reward, extrinsic_reward; /* HFOGameState's doubles, as Evaluate() sums them (:181-182) */
  int32_t steps;                         /* HFOGameState::steps (counts the initial update) */
  int32_t status, worker, reserved;      /* status: the HFO status that ended it (4 also: max_steps reached) */
  int64_t step_index;                    /* the handle's observe count at which the episode ended (first observe = 1) */
} dqnhip_env_episode;

/* N workers whose states come from the caller.  first_states_host [N,S] are the states after the
 * forced DASH(0,0) (src/dqn_main.cpp:103-105): every worker gets HFOGameState() and the initial
 * update with player on ball 0.  cfg->p_end / p_goal are ignored; cfg->seed keys the epsilon draws
 * and the random ActorOutputs.  The per-worker draw counter starts where a synthetic handle's stands
 * after its reset and moves by the same rule (1 per step, 2 on a step that ends an episode), so an
 * external handle fed a synthetic handle's stream draws what that handle draws.  max_steps should be
 * >= the simulator's frames-per-trial: an episode that reaches it while IN_GAME is closed as
 * OUT_OF_TIME and counted in dqnhip_env_debug_read(e, "truncated").
 * flags: 0, or DQNHIP_ENV_NO_RECORD — no episode rows are allocated, the replay memory is never
 * written (and the workers*max_steps < replay capacity condition of a recording handle is waived). */
int dqnhip_env_create_external(dqnhip_handle h, const dqnhip_env_config* cfg, int32_t flags,
                               const float* first_states_host, dqnhip_env_handle* out);

/* SelectAction(state, epsilon) + GetAction for every worker (src/dqn.cpp:684-711, 196-208): one
 * batched actor forward over the N current states (in the learner's acting precision,
 * dqnhip_set_act_precision), one epsilon draw per worker, the random or greedy ActorOutput.  The
 * chosen row opens the worker's next transition and goes to the caller: action [N] (GetAction's
 * index: 0 DASH, 1 TURN, 2 TACKLE, 3 KICK), args [N,2] (arg1, arg2; arg2 = 0 where the action has
 * one parameter), actor_out [N,10] (may be NULL).  act and observe alternate: a second act before
 * the observe fails.  dqnhip_env_act takes host arrays and blocks; dqnhip_env_act_device takes
 * device pointers and is asynchronous on the learner's stream. */
int dqnhip_env_act(dqnhip_env_handle e, float epsilon, int32_t* action, float* args, float* actor_out);
int dqnhip_env_act_device(dqnhip_env_handle e, float epsilon, int32_t* action_dev, float* args_dev,
                          float* actor_out_dev);

/* What the simulator answered (the hfo.step() inside HFOGameState::update, src/hfo_game.cpp:122-173):
 * next_states [N,S] dense, status [N] (the HFO enum: 0 IN_GAME, 1 GOAL, 2 CAPTURED_BY_DEFENSE,
 * 3 OUT_OF_BOUNDS, 4 OUT_OF_TIME), player_on_ball [N].  next_states[w] is the state worker w shows
 * the actor next: the successor state while status[w] is IN_GAME, otherwise the FIRST STATE OF THE
 * WORKER'S NEXT EPISODE — a terminal transition has no next state (src/dqn_main.cpp:138-140) and
 * the update zeroes the deltas a terminal row would feed (src/hfo_game.cpp:164-168).  Per worker:
 * HFOGameState::update + reward, the transition's reward; on a terminal status an episode record,
 * LabelTransitions + AddTransitions in worker order (not with DQNHIP_ENV_NO_RECORD), and a fresh
 * HFOGameState with the initial update on the new first state.  A status of 5 (SERVER_DOWN) or
 * outside 0..5 closes the episode and raises a sticky flag: the next dqnhip_env_stats /
 * dqnhip_env_read_episodes fails with "Server Down!" / "status out of range"
 * (src/hfo_game.cpp:124-126).  A recording handle's observe changes the replay memory on the device
 * as dqnhip_env_step does: a chain started by dqnhip_update_chained ends there.  Both variants are
 * asynchronous; the host variant has copied its arguments when it returns. */
int dqnhip_env_observe(dqnhip_env_handle e, const float* next_states, const int32_t* status,
                       const int32_t* player_on_ball);
int dqnhip_env_observe_device(dqnhip_env_handle e, const float* next_states_dev, const int32_t* status_dev,
                              const int32_t* player_on_ball_dev);

/* Blocks; hands out up to cap records of finished episodes, ordered by (step_index, worker), each
 * once: what does not fit stays for the next call.  The device keeps the last 8 records of each
 * worker between two calls; *dropped (may be NULL) is the number overwritten unread since creation. */
int dqnhip_env_read_episodes(dqnhip_env_handle e, dqnhip_env_episode* out, int32_t cap, int32_t* n_out,
                             int64_t* dropped);

#ifdef __cplusplus
}
#endif
#endif /* DQNHIP_ENV_H_ */
