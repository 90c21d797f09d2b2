"""Host-side mirror of the reference's `dqn::DQN` (src/dqn.hpp:56-134) for the hot
path, over the C-ABI of include/dqnhip.h.  Method names, argument meaning and error
behaviour follow the reference; where the reference aborts through glog CHECK /
LOG(FATAL) this raises `DQNFatal`.

PyTorch is not used here at all — device memory and streams live inside the native
library; torch only appears in parallel.py (torch.distributed over RCCL).
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from . import capi
from .capi import ACTOR, CRITIC, ACTOR_TARGET, CRITIC_TARGET, KIND_W, KIND_M, KIND_V, KIND_G

kActionSize = 4          # src/dqn.hpp:20
kActionParamSize = 6     # src/dqn.hpp:21
kStateInputCount = 1     # src/dqn.hpp:18
DASH, TURN, TACKLE, KICK = 0, 1, 2, 3   # hfo::action_t values pinned by src/dqn.cpp:181-186

Action = namedtuple("Action", "action arg1 arg2")          # src/hfo_game.hpp:7-11
Transition = namedtuple("Transition", "state actor_output reward on_policy_target next_state")
# next_state is None for terminal transitions (boost::none, src/dqn.cpp:878)


class DQNFatal(RuntimeError):
    """The reference's CHECK/LOG(FATAL) abort, as an exception."""


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(capi.fp)


def GetParamOffset(action, arg_num=0):
    """src/dqn.cpp:162-178."""
    if arg_num < 0 or arg_num > 1:
        return -1
    if action == DASH:
        return arg_num
    if action == TURN:
        return 2 if arg_num == 0 else -1
    if action == TACKLE:
        return 3 if arg_num == 0 else -1
    if action == KICK:
        return 4 + arg_num
    raise DQNFatal("Unrecognized action: %r" % (action,))


def GetAction(actor_output):
    """src/dqn.cpp:196-208: argmax over the 4 logits with TACKLE masked to -99999
    (std::max_element: the first maximum wins), then the chosen action's parameters."""
    ao = np.asarray(actor_output, dtype=np.float32)
    copy = ao[:kActionSize].copy()
    copy[TACKLE] = -99999
    act = int(np.argmax(copy))                 # np.argmax also returns the first maximum
    o1 = GetParamOffset(act, 0)
    assert o1 >= 0
    o2 = GetParamOffset(act, 1)
    return Action(act, float(ao[kActionSize + o1]), 0.0 if o2 < 0 else float(ao[kActionSize + o2]))


def PrintActorOutput(ao):
    """src/dqn.cpp:210-216."""
    f = lambda v: "%f" % v
    return ("Dash(" + f(ao[4]) + ", " + f(ao[5]) + ")=" + f(ao[0]) + ", Turn(" + f(ao[6]) + ")=" + f(ao[1])
            + ", Tackle(" + f(ao[7]) + ")=" + f(ao[2]) + ", Kick(" + f(ao[8]) + ", " + f(ao[9]) + ")=" + f(ao[3]))


class DQN:
    supports_split_phase0 = True        # dqnhip_update_phase accepts 10 / 11 (parallel.DataParallelUpdate)
    """Device-resident learner with the reference's method surface.

    Constructor arguments replace the reference's SolverParameter pair + gflags
    (src/dqn.cpp:21-31, src/dqn_main.cpp:249-262); defaults are the reference's.
    """

    def __init__(self, state_size, minibatch=32, hidden=(1024, 512, 256, 128), memory=500000,
                 gamma=0.99, beta=0.5, tau=0.001, soft_update_freq=1, actor_lr=1e-5, critic_lr=1e-3,
                 momentum=0.95, momentum2=0.999, clip_grad=10.0, memory_threshold=1000, seed=1,
                 device=0, dp_world=1, dp_rank=0, use_graph=False, stream=None, grad_arena=None,
                 grad_arena_bytes=0, tid=0, save_path="state/dqn", precision="fp32", loss_scale=0.0, tuning=0,
                 loss_scale_mode="static", loss_scale_growth_interval=None, loss_scale_min_mult=None, loss_scale_max_mult=None,
                 act_precision="fp32", solver="Adam", rms_decay=0.99, delta=None,
                 lr_policy="fixed", lr_gamma=0.0, lr_power=0.0, lr_stepsize=0, lr_stepvalues=(), lr_max_iter=0,
                 weight_decay=0.0, regularization="L2"):
        self.lib = capi.load()
        cfg = capi.Config()
        self.lib.dqnhip_default_config(C.byref(cfg), state_size)
        cfg.minibatch = minibatch
        cfg.num_hidden = len(hidden)
        for i in range(capi.MAX_HIDDEN):
            cfg.hidden[i] = hidden[i] if i < len(hidden) else 0
        cfg.replay_capacity = memory
        cfg.soft_update_freq = soft_update_freq
        cfg.gamma, cfg.beta, cfg.tau = gamma, beta, tau
        cfg.actor_lr, cfg.critic_lr = actor_lr, critic_lr
        cfg.momentum, cfg.momentum2, cfg.clip_gradients = momentum, momentum2, clip_grad
        cfg.device, cfg.dp_world, cfg.dp_rank, cfg.use_graph = device, dp_world, dp_rank, int(use_graph)
        cfg.seed = seed
        cfg.stream = stream
        cfg.grad_arena = grad_arena
        cfg.grad_arena_bytes = grad_arena_bytes
        cfg.precision = {"fp32": 0, "fp16": 1}[precision]
        cfg.loss_scale = loss_scale
        cfg.tuning_flags = int(tuning)                  # capi.TUNE_* bits: alternative schedules of the same arithmetic
        # fp16 learner: "dynamic" lets the optimiser launches halve / double a per-net multiplier of the loss scales (None: the header's defaults)
        cfg.loss_scale_mode = {"static": capi.LOSS_SCALE_STATIC, "dynamic": capi.LOSS_SCALE_DYNAMIC}[loss_scale_mode]
        if loss_scale_growth_interval is not None:
            cfg.loss_scale_growth_interval = int(loss_scale_growth_interval)
        if loss_scale_min_mult is not None:
            cfg.loss_scale_min_mult = loss_scale_min_mult
        if loss_scale_max_mult is not None:
            cfg.loss_scale_max_mult = loss_scale_max_mult
        # Caffe's solver type string (the reference driver's -solver); AdaGrad and RMSProp need momentum=0, as in Caffe
        if solver not in capi.SOLVERS:
            raise DQNFatal("Unknown solver type: %s (known types: %s)" % (solver, ", ".join(capi.SOLVERS)))
        cfg.solver_type, cfg.rms_decay = capi.SOLVERS.index(solver), rms_decay
        if delta is not None:
            cfg.delta = delta
        # Caffe's lr_policy / weight_decay (SolverParameter); one schedule and one decay serve both nets, the base rates are actor_lr / critic_lr
        if lr_policy not in capi.LR_POLICIES:
            raise DQNFatal("Unknown learning rate policy: %s (known policies: %s)" % (lr_policy, ", ".join(capi.LR_POLICIES)))
        if regularization not in capi.REGULARIZATIONS:
            raise DQNFatal("Unknown regularization type: %s (known types: %s)" % (regularization, ", ".join(capi.REGULARIZATIONS)))
        if len(lr_stepvalues) > capi.LR_MAX_STEPVALUES:
            raise DQNFatal("lr_policy multistep: 1 to %d stepvalues required (got %d)" % (capi.LR_MAX_STEPVALUES, len(lr_stepvalues)))
        cfg.lr_policy, cfg.lr_gamma, cfg.lr_power = capi.LR_POLICIES.index(lr_policy), lr_gamma, lr_power
        cfg.lr_stepsize, cfg.lr_max_iter, cfg.lr_n_stepvalue = int(lr_stepsize), int(lr_max_iter), len(lr_stepvalues)
        for i, sv in enumerate(lr_stepvalues):
            cfg.lr_stepvalue[i] = int(sv)
        cfg.weight_decay, cfg.regularization_type = weight_decay, capi.REGULARIZATIONS.index(regularization)
        self.cfg = cfg
        self.h = capi.H()
        self._ck(self.lib.dqnhip_create(C.byref(cfg), C.byref(self.h)))
        self.state_size_ = state_size
        self.kMinibatchSize = minibatch
        self.memory_threshold = memory_threshold        # FLAGS_memory_threshold, src/dqn.cpp:26
        self.gamma_ = gamma
        self.tid_ = tid
        self.save_path_ = save_path
        self.unum_ = 0
        self.random_engine = np.random.default_rng(seed)   # stands in for std::mt19937
        self.smoothed_critic_loss_ = 0.0
        self.smoothed_actor_loss_ = 0.0
        self.last_snapshot_iter_ = 0
        self.snapshot_freq = 10000                      # FLAGS_snapshot_freq, src/dqn.cpp:28
        self.select_actions_cap = 0                     # 0: the reference's cap (the minibatch, src/dqn.cpp:699); -1: none; n: n
        if act_precision != "fp32":
            try:
                self.set_act_precision(act_precision)
            except Exception:
                self.close()
                raise

    # -- plumbing -----------------------------------------------------------------
    @staticmethod
    def grad_arena_bytes(state_size, minibatch, hidden, precision="fp32"):
        lib = capi.load()
        cfg = capi.Config()
        lib.dqnhip_default_config(C.byref(cfg), state_size)
        cfg.minibatch = minibatch
        cfg.precision = {"fp32": 0, "fp16": 1}[precision]
        cfg.num_hidden = len(hidden)
        for i, hsz in enumerate(hidden):
            cfg.hidden[i] = hsz
        return lib.dqnhip_grad_arena_bytes(C.byref(cfg))

    @property
    def solver(self):
        """Caffe's type string of this learner's solver (dqnhip_solver_name)."""
        return self.lib.dqnhip_solver_name(self.cfg.solver_type).decode()

    def learning_rate(self, net):
        """The rate net's next optimiser step applies (dqnhip_get_learning_rate: the lr policy at the net's current iteration)."""
        out = C.c_float()
        self._ck(self.lib.dqnhip_get_learning_rate(self.h, int(net), C.byref(out)))
        return out.value

    def _ck(self, rc):
        if rc != 0:
            raise DQNFatal(self.lib.dqnhip_last_error().decode())

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self._ck(self.lib.dqnhip_destroy(self.h))      # refuses while sharers exist
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- accessors (src/dqn.hpp:112, 127-134) ------------------------------------------
    def memory_size(self):
        n = C.c_int32()
        self._ck(self.lib.dqnhip_memory_size(self.h, C.byref(n)))
        return n.value

    def _iters(self):
        a, c = C.c_int32(), C.c_int32()
        self._ck(self.lib.dqnhip_get_iters(self.h, C.byref(a), C.byref(c)))
        return a.value, c.value

    def actor_iter(self):
        return self._iters()[0]

    def critic_iter(self):
        return self._iters()[1]

    def max_iter(self):
        return max(self._iters())

    def min_iter(self):
        return min(self._iters())

    def set_iters(self, actor_iter, critic_iter):
        self._ck(self.lib.dqnhip_set_iters(self.h, actor_iter, critic_iter))

    def state_size(self):
        return self.state_size_

    def save_path(self):
        return self.save_path_

    def unum(self):
        return self.unum_

    def set_unum(self, unum):
        self.unum_ = unum

    # -- replay memory -------------------------------------------------------------------
    def ClearReplayMemory(self):
        self._ck(self.lib.dqnhip_clear_memory(self.h))

    def LabelTransitions(self, transitions):
        """src/dqn.cpp:783-797: fills on_policy_target by the reverse discounted scan;
        returns the relabelled list (the reference mutates in place)."""
        if len(transitions) == 0:
            raise DQNFatal("Need at least one transition to label.")
        r = _f32([t.reward for t in transitions])
        mc = np.empty_like(r)
        self._ck(self.lib.dqnhip_label_transitions(self.gamma_, _p(r), r.size, _p(mc)))
        return [t._replace(on_policy_target=float(m)) for t, m in zip(transitions, mc)]

    def _pack(self, transitions):
        S = self.state_size_
        n = len(transitions)
        s = np.empty((n, S), np.float32); nx = np.zeros((n, S), np.float32)
        a = np.empty((n, 10), np.float32); r = np.empty(n, np.float32); mc = np.empty(n, np.float32)
        term = np.zeros(n, np.uint8)
        for i, t in enumerate(transitions):
            if len(t.state) != S:
                raise DQNFatal("state size %d != %d" % (len(t.state), S))
            s[i] = t.state; a[i] = t.actor_output; r[i] = t.reward; mc[i] = t.on_policy_target
            if t.next_state is None:
                term[i] = 1
            else:
                nx[i] = t.next_state
        return s, a, r, mc, nx, term

    def AddTransition(self, transition):
        """src/dqn.cpp:768-773."""
        s, a, r, mc, nx, term = self._pack([transition])
        self._ck(self.lib.dqnhip_add_transition(self.h, _p(s), _p(a), float(r[0]), float(mc[0]), _p(nx), int(term[0])))

    def AddTransitions(self, transitions):
        """src/dqn.cpp:775-781."""
        s, a, r, mc, nx, term = self._pack(transitions)
        self.add_transitions_arrays(s, a, r, mc, nx, term)

    def add_transitions_arrays(self, s, a, r, mc, nx, term):
        """AddTransitions on already-packed arrays ([n,S], [n,10], [n], [n], [n,S], [n] u8)."""
        s, a, r, mc, nx = _f32(s), _f32(a), _f32(r), _f32(mc), _f32(nx)
        term = np.ascontiguousarray(term, dtype=np.uint8)
        self._ck(self.lib.dqnhip_add_transitions(self.h, _p(s), _p(a), _p(r), _p(mc), _p(nx),
                                                 term.ctypes.data_as(capi.up), r.size))

    def read_memory(self, first, n):
        S = self.state_size_
        s = np.empty((n, S), np.float32); nx = np.empty((n, S), np.float32)
        a = np.empty((n, 10), np.float32); r = np.empty(n, np.float32); mc = np.empty(n, np.float32)
        t = np.empty(n, np.uint8)
        self._ck(self.lib.dqnhip_read_memory(self.h, first, n, _p(s), _p(a), _p(r), _p(mc), _p(nx),
                                             t.ctypes.data_as(capi.up)))
        return s, a, r, mc, nx, t

    # -- snapshot / restore (src/dqn.cpp:525-620) ---------------------------------------------------
    def Snapshot(self, snapshot_prefix=None, remove_old=None, snapshot_memory=None, wait=True, compress_threads=0):
        """DQN::Snapshot(): `<prefix>_{actor,critic}_iter_N.{caffemodel,solverstate}` (+
        `<prefix>_iter_N.replaymemory`) in Caffe's binary protobuf layout.  With no arguments:
        Snapshot(save_path_, FLAGS_remove_old_snapshots=True, FLAGS_snapshot_memory=True).
        wait=False: dqnhip_snapshot_async — the same files under the same names, frozen on the device at this point of the stream and
        written by the learner's writer thread (the replay memory deflated by `compress_threads` threads, 0: 8) while training goes
        on; snapshot_wait() joins it and reports its status."""
        prefix = self.save_path_ if snapshot_prefix is None else snapshot_prefix
        remove_old = True if remove_old is None and snapshot_prefix is None else bool(remove_old)
        snapshot_memory = True if snapshot_memory is None else bool(snapshot_memory)
        if wait:
            self._ck(self.lib.dqnhip_snapshot(self.h, os.fsencode(self.save_path_), os.fsencode(prefix),
                                              int(remove_old), int(snapshot_memory)))
        else:
            self._ck(self.lib.dqnhip_snapshot_async(self.h, os.fsencode(self.save_path_), os.fsencode(prefix),
                                                    int(remove_old), int(snapshot_memory), int(compress_threads)))
        self.last_snapshot_iter_ = self.max_iter()

    def snapshot_wait(self):
        """dqnhip_snapshot_wait: joins an asynchronous snapshot in flight; raises if it failed.  -> (actor_iter, critic_iter) its files
        are named by ((0, 0) when this learner never snapshotted asynchronously)."""
        ia, ic = C.c_int32(), C.c_int32()
        self._ck(self.lib.dqnhip_snapshot_wait(self.h, C.byref(ia), C.byref(ic)))
        return ia.value, ic.value

    def snapshot_done(self):
        """dqnhip_snapshot_poll: True when no asynchronous snapshot is in flight.  Never blocks."""
        done = C.c_int32()
        self._ck(self.lib.dqnhip_snapshot_poll(self.h, C.byref(done)))
        return bool(done.value)

    def RestoreActorSolver(self, actor_solver):
        self._ck(self.lib.dqnhip_solver_restore(self.h, ACTOR, os.fsencode(actor_solver)))
        self.last_snapshot_iter_ = self.max_iter()

    def RestoreCriticSolver(self, critic_solver):
        self._ck(self.lib.dqnhip_solver_restore(self.h, CRITIC, os.fsencode(critic_solver)))
        self.last_snapshot_iter_ = self.max_iter()

    def LoadActorWeights(self, actor_weights):
        self._ck(self.lib.dqnhip_load_caffemodel(self.h, ACTOR, os.fsencode(actor_weights)))

    def LoadCriticWeights(self, critic_weights):
        self._ck(self.lib.dqnhip_load_caffemodel(self.h, CRITIC, os.fsencode(critic_weights)))

    def SnapshotReplayMemory(self, filename):
        """src/dqn.cpp:1146-1178: gzip `.replaymemory` file in the reference's byte layout."""
        self._ck(self.lib.dqnhip_snapshot_replay_memory(self.h, os.fsencode(filename)))

    def LoadReplayMemory(self, filename):
        """src/dqn.cpp:1180-1226."""
        self._ck(self.lib.dqnhip_load_replay_memory(self.h, os.fsencode(filename)))

    # -- acting (src/dqn.cpp:664-711) -------------------------------------------------------
    def GetRandomActorOutput(self):
        g = self.random_engine
        ao = np.empty(10, np.float32)
        ao[0:4] = g.uniform(-1.0, 1.0, 4)
        ao[4] = g.uniform(-100.0, 100.0)
        ao[5] = g.uniform(-180.0, 180.0); ao[6] = g.uniform(-180.0, 180.0); ao[7] = g.uniform(-180.0, 180.0)
        ao[8] = g.uniform(0.0, 100.0)
        ao[9] = g.uniform(-180.0, 180.0)
        return ao

    def set_act_precision(self, precision):
        """"fp32" (default): acting runs the exact-fp32 kernels on the master weights.  "fp16" (fp16 learners only): acting computes
        what the update's own forward passes compute, on the fp16 weight mirrors (dqnhip_set_act_precision).  Launches nothing."""
        if precision not in ("fp32", "fp16"):
            raise DQNFatal("act_precision must be 'fp32' or 'fp16' (got %r)" % (precision,))
        self._ck(self.lib.dqnhip_set_act_precision(self.h, {"fp32": capi.FP32, "fp16": capi.FP16}[precision]))

    @property
    def act_precision(self):
        v = C.c_int32()
        self._ck(self.lib.dqnhip_get_act_precision(self.h, C.byref(v)))
        return "fp16" if v.value == capi.FP16 else "fp32"

    def SelectActionGreedily(self, states_batch, net=ACTOR):
        s = _f32(states_batch).reshape(-1, self.state_size_)
        out = np.empty((s.shape[0], 10), np.float32)
        self._ck(self.lib.dqnhip_select_actions_net(self.h, net, _p(s), s.shape[0], _p(out)))
        return out

    def SelectActions(self, states_batch, epsilon):
        """src/dqn.cpp:695-711: ONE epsilon draw for the whole batch.  The reference's `CHECK_LE(states_batch.size(),
        kMinibatchSize)` (:699) holds with this learner's minibatch; `select_actions_cap` widens it (-1: any batch — the
        device path has no MemoryData layer whose width would bound it; n > 0: that many)."""
        if not (0.0 <= epsilon <= 1.0):
            raise DQNFatal("CHECK failed: epsilon >= 0.0 && epsilon <= 1.0")
        s = _f32(states_batch).reshape(-1, self.state_size_)
        cap = self.kMinibatchSize if self.select_actions_cap == 0 else self.select_actions_cap
        if cap >= 0 and s.shape[0] > cap:
            raise DQNFatal("CHECK failed: states_batch.size() <= kMinibatchSize (%d vs. %d)" % (s.shape[0], cap))
        if self.random_engine.uniform(0.0, 1.0) < epsilon:
            return np.stack([self.GetRandomActorOutput() for _ in range(s.shape[0])])
        return self.SelectActionGreedily(s)

    def SelectAction(self, input_states, epsilon):
        return self.SelectActions(np.asarray(input_states, np.float32).reshape(1, -1), epsilon)[0]

    def SampleAction(self, actor_output):
        """src/dqn.cpp:180-194: sample the discrete action with probabilities max(0, logit+1),
        TACKLE removed; not used on the reference's default path."""
        ao = np.asarray(actor_output, dtype=np.float32)
        p = np.array([max(0.0, ao[DASH] + 1.0), max(0.0, ao[TURN] + 1.0), 0.0, max(0.0, ao[KICK] + 1.0)])
        act = int(self.random_engine.choice(4, p=p / p.sum()))
        o1, o2 = GetParamOffset(act, 0), GetParamOffset(act, 1)
        return Action(act, float(ao[kActionSize + o1]), 0.0 if o2 < 0 else float(ao[kActionSize + o2]))

    def SampleStatesFromMemory(self, n, idx=None):
        """src/dqn.cpp:511-523: the states of n uniformly sampled transitions ([n,S]); idx = the
        explicit form of SampleTransitionsFromMemory, None = device draw."""
        out = np.empty((n, self.state_size_), np.float32)
        ip = None
        if idx is not None:
            i = np.ascontiguousarray(idx, dtype=np.int32)
            if i.size != n:
                raise DQNFatal("need %d indices" % n)
            ip = i.ctypes.data_as(capi.ip)
        self._ck(self.lib.dqnhip_sample_states(self.h, ip, n, _p(out)))
        return out

    def getActorOutput(self, batch_size, net=ACTOR):
        """src/dqn.cpp:719-732: the actor's output blobs as its last minibatch forward left them."""
        out = np.empty((batch_size, 10), np.float32)
        self._ck(self.lib.dqnhip_get_actor_output(self.h, net, batch_size, _p(out)))
        return out

    def CriticForward(self, states_batch, action_batch, net=CRITIC):
        s = _f32(states_batch).reshape(-1, self.state_size_)
        a = _f32(action_batch).reshape(-1, 10)
        if s.shape[0] != a.shape[0]:
            raise DQNFatal("CHECK_EQ(states_batch.size(), action_batch.size())")
        q = np.empty(s.shape[0], np.float32)
        self._ck(self.lib.dqnhip_critic_forward(self.h, net, _p(s), _p(a), s.shape[0], _p(q)))
        return q

    def EvaluateAction(self, input_states, action):
        """src/dqn.cpp:688-693."""
        return float(self.CriticForward(np.asarray(input_states).reshape(1, -1), np.asarray(action).reshape(1, -1))[0])

    # -- the update (src/dqn.cpp:799-972) ---------------------------------------------------------
    def UpdateActorCritic(self, idx=None):
        """One update; idx = explicit sampled indices or None for on-device
        sampling.  Returns (critic_loss, avg_q) like the reference."""
        loss, avgq = C.c_float(), C.c_float()
        keep, ip = self._idx(idx)
        self._ck(self.lib.dqnhip_update(self.h, ip, C.byref(loss), C.byref(avgq)))
        return loss.value, avgq.value

    def _idx(self, idx):
        """B explicit sampled indices as an int32 pointer (the C side reads exactly kMinibatchSize)."""
        if idx is None:
            return None, None
        i = np.ascontiguousarray(idx, dtype=np.int32)
        if i.size != self.kMinibatchSize:
            raise DQNFatal("need %d indices, got %d" % (self.kMinibatchSize, i.size))
        return i, i.ctypes.data_as(capi.ip)

    def UpdateActorCriticChained(self, idx, idx_next=None):
        """dqnhip_update_chained: this update on idx; idx_next = the indices the NEXT call will bring (its gather and first layers then
        ride in this update's optimiser launches).  Same results as UpdateActorCritic(idx)."""
        loss, avgq = C.c_float(), C.c_float()
        keep, ip = self._idx(idx)
        keep2, ip2 = self._idx(idx_next)
        self._ck(self.lib.dqnhip_update_chained(self.h, ip, ip2, C.byref(loss), C.byref(avgq)))
        return loss.value, avgq.value

    def UpdateActorCriticPipelined(self, idx=None):
        """dqnhip_update_pipelined: enqueue this update, return (critic_loss, avg_q) of the PREVIOUS one."""
        loss, avgq = C.c_float(), C.c_float()
        keep, ip = self._idx(idx)
        self._ck(self.lib.dqnhip_update_pipelined(self.h, ip, C.byref(loss), C.byref(avgq)))
        return loss.value, avgq.value

    def update_async(self, idx=None):
        keep, ip = self._idx(idx)
        self._ck(self.lib.dqnhip_update_async(self.h, ip))

    def update_async_n(self, n):
        """n updates with on-device sampling in one call (dqnhip_update_async_n)."""
        self._ck(self.lib.dqnhip_update_async_n(self.h, int(n)))

    def update_indexed_n(self, idx):
        """dqnhip_update_indexed_n: one update per row of idx ([n, B] int32), enqueued as multi-update graphs without waiting;
        the state n UpdateActorCritic(idx[t]) calls leave.  collect_stats() returns the pairs."""
        i = np.ascontiguousarray(idx, dtype=np.int32)
        if i.size and (i.ndim != 2 or i.shape[1] != self.kMinibatchSize):
            raise DQNFatal("need [n, %d] indices, got %r" % (self.kMinibatchSize, i.shape))
        n = i.shape[0] if i.ndim == 2 else 0
        self._ck(self.lib.dqnhip_update_indexed_n(self.h, i.ctypes.data_as(capi.ip) if n else None, n))

    def collect_stats(self, cap=None, out=None):
        """dqnhip_collect_stats: waits for the indexed updates enqueued so far; the (critic_loss, avg_q) pairs not yet collected, in
        update order (at most cap of them; None: all).  A flagged update raises DQNFatal AFTER the pairs were appended to `out`
        (pass a list to keep them)."""
        pairs = [] if out is None else out
        while cap is None or cap > 0:
            k = 256 if cap is None else min(cap, 256)
            loss, avgq, n = np.empty(k, np.float32), np.empty(k, np.float32), C.c_int32()
            rc = self.lib.dqnhip_collect_stats(self.h, _p(loss), _p(avgq), k, C.byref(n))
            pairs.extend((float(np.float32(a)), float(np.float32(b))) for a, b in zip(loss[:n.value], avgq[:n.value]))
            self._ck(rc)
            if cap is not None:
                cap -= n.value
            if n.value < k:
                break
        return pairs

    def update_phase(self, phase, idx=None):
        keep, ip = self._idx(idx)
        self._ck(self.lib.dqnhip_update_phase(self.h, phase, ip))

    def update_abort(self):
        """Abandon a phased update whose exchange step failed (the next update starts afresh)."""
        self._ck(self.lib.dqnhip_update_abort(self.h))

    def apply_update(self, net):
        """Solver::ApplyUpdate of one net on the gradient in its arena (src/dqn.cpp:904 tail, :964-965)."""
        self._ck(self.lib.dqnhip_apply_update(self.h, net))

    def apply_update_sharded(self, net, world):
        """The same step, evaluated as a `world`-rank group with a sharded optimiser evaluates it (one slice after the other)."""
        self._ck(self.lib.dqnhip_apply_update_sharded(self.h, net, int(world)))

    # -- native data parallelism (RCCL inside the library, include/dqnhip.h dqnhip_dp_*) -------
    @staticmethod
    def dp_unique_id():
        lib = capi.load()
        buf = C.create_string_buffer(capi.DP_ID_BYTES)
        if lib.dqnhip_dp_unique_id(buf, capi.DP_ID_BYTES) != 0:
            raise DQNFatal(lib.dqnhip_last_error().decode())
        return buf.raw

    @staticmethod
    def _dp_flags(per_layer, half_grads, shard_opt=False, unverified_ok=False):
        return ((capi.DP_PER_LAYER if per_layer else 0) | (capi.DP_HALF_GRADS if half_grads else 0) |
                (capi.DP_SHARD_OPT if shard_opt else 0) | (capi.DP_UNVERIFIED_OK if unverified_ok else 0))

    def dp_init(self, unique_id, per_layer=False, half_grads=False, shard_opt=False, unverified_ok=False):
        """unverified_ok: per_layer / shard_opt have never run on more than one rank; a real group must ask for them explicitly."""
        assert len(unique_id) == capi.DP_ID_BYTES
        buf = C.create_string_buffer(bytes(unique_id), capi.DP_ID_BYTES)
        self._ck(self.lib.dqnhip_dp_init(self.h, buf, capi.DP_ID_BYTES, self._dp_flags(per_layer, half_grads, shard_opt, unverified_ok)))

    def dp_init_file(self, path, per_layer=False, timeout_s=120, half_grads=False, shard_opt=False, unverified_ok=False):
        self._ck(self.lib.dqnhip_dp_init_file(self.h, os.fsencode(path), self._dp_flags(per_layer, half_grads, shard_opt, unverified_ok), int(timeout_s)))

    @staticmethod
    def dp_info():
        """(RCCL version, path of the librccl this process resolved): a group must not mix builds (dqnhip_dp_init checks)."""
        lib = capi.load()
        v = C.c_int32()
        buf = C.create_string_buffer(4096)
        if lib.dqnhip_dp_info(C.byref(v), buf, 4096) != 0:
            raise DQNFatal(lib.dqnhip_last_error().decode())
        return v.value, os.fsdecode(buf.value)

    def dp_gather_state(self):
        """sharded optimiser: all-gather of the Adam history (collective; no-op otherwise)"""
        self._ck(self.lib.dqnhip_dp_gather_state(self.h))

    def dp_graph_active(self):
        v = C.c_int32()
        self._ck(self.lib.dqnhip_dp_graph_active(self.h, C.byref(v)))
        return bool(v.value)

    def dp_destroy(self):
        self._ck(self.lib.dqnhip_dp_destroy(self.h))

    def dp_broadcast_params(self, root=0):
        self._ck(self.lib.dqnhip_dp_broadcast_params(self.h, int(root)))

    def dp_update(self, idx=None):
        keep, ip = self._idx(idx)
        self._ck(self.lib.dqnhip_dp_update(self.h, ip))

    def dp_update_n(self, n):
        """n data-parallel updates with on-device sampling in one call (every rank: the same n)."""
        self._ck(self.lib.dqnhip_dp_update_n(self.h, int(n)))

    def skipped_steps(self):
        n = C.c_int64()
        self._ck(self.lib.dqnhip_skipped_steps(self.h, C.byref(n)))
        return n.value

    def loss_scale_state(self):
        """dqnhip_get_loss_scale as a dict: mode, mult_critic / mult_actor, good_*, backoffs_*, growths_*, skipped_steps."""
        s = capi.LossScaleState()
        self._ck(self.lib.dqnhip_get_loss_scale(self.h, C.byref(s)))
        d = {name: getattr(s, name) for name, _ in capi.LossScaleState._fields_ if name not in ("struct_size", "reserved", "mode")}
        d["mode"] = "dynamic" if s.mode == capi.LOSS_SCALE_DYNAMIC else "static"
        return d

    def set_loss_scale(self, mult_critic, mult_actor):
        """Dynamic mode: sets both multipliers (powers of two inside the configured bounds) and zeroes the finite-step counters."""
        self._ck(self.lib.dqnhip_set_loss_scale(self.h, float(mult_critic), float(mult_actor)))

    def read_stats(self):
        loss, avgq = C.c_float(), C.c_float()
        self._ck(self.lib.dqnhip_read_stats(self.h, C.byref(loss), C.byref(avgq)))
        return loss.value, avgq.value

    def Update(self, loss_display_iter=1000):
        """src/dqn.cpp:799-826 (snapshotting is in snapshot.py)."""
        if self.memory_size() < self.memory_threshold:
            return None
        critic_loss, avg_q = self.UpdateActorCritic()
        logs = []
        if self.critic_iter() % loss_display_iter == 0:
            logs.append("[Agent%d] Critic Iteration %d, loss = %g" % (self.tid_, self.critic_iter(), self.smoothed_critic_loss_))
            self.smoothed_critic_loss_ = 0.0
        self.smoothed_critic_loss_ += critic_loss / float(loss_display_iter)
        if self.actor_iter() % loss_display_iter == 0:
            logs.append("[Agent%d] Actor Iteration %d, avg_q_value = %g" % (self.tid_, self.actor_iter(), self.smoothed_actor_loss_))
            self.smoothed_actor_loss_ = 0.0
        self.smoothed_actor_loss_ += avg_q / float(loss_display_iter)
        for line in logs:
            print(line)
        # periodic snapshot (src/dqn.cpp:818-825)
        if (self.critic_iter() >= self.last_snapshot_iter_ + self.snapshot_freq or
                self.actor_iter() >= self.last_snapshot_iter_ + self.snapshot_freq):
            self.Snapshot()
        return critic_loss, avg_q

    def Benchmark(self, iterations=1000, warmup=0):
        """src/dqn.cpp:487-498; returns the average update time in ms."""
        ms = C.c_float()
        self._ck(self.lib.dqnhip_benchmark(self.h, warmup, iterations, C.byref(ms)))
        return ms.value

    def BenchmarkBlocking(self, iterations=1000, warmup=50, seed=1, pipelined=False):
        """DQN::Benchmark as the drop-in's caller sees it: host-drawn indices + a (loss, avg_q) read-back per
        update (blocking, or one-deep pipelined; 2: the chained form; 3: deferred — a dqnhip_update_indexed_n every sixteen
        updates, a dqnhip_collect_stats every 1000); average wall-clock ms per update."""
        ms = C.c_float()
        self._ck(self.lib.dqnhip_benchmark_blocking(self.h, warmup, iterations, seed, int(pipelined), C.byref(ms)))
        return ms.value

    # -- parameters ------------------------------------------------------------------------------------
    def param_count(self, net):
        n = C.c_size_t()
        self._ck(self.lib.dqnhip_param_count(self.h, net, C.byref(n)))
        return n.value

    def get_params(self, net, kind=KIND_W):
        out = np.empty(self.param_count(net), np.float32)
        self._ck(self.lib.dqnhip_get_params(self.h, net, kind, _p(out), out.size))
        return out

    def set_params(self, net, arr, kind=KIND_W):
        a = _f32(arr)
        self._ck(self.lib.dqnhip_set_params(self.h, net, kind, _p(a), a.size))

    def CloneNet(self, net):
        """src/dqn.cpp:1022-1035: hard copy online -> target."""
        self._ck(self.lib.dqnhip_clone_to_target(self.h, net))

    def ShareParameters(self, other, num_actor_layers_to_share, num_critic_layers_to_share):
        """src/dqn.cpp:1047-1078: `other`'s first layers (and its targets') use this learner's weights."""
        self._ck(self.lib.dqnhip_share_parameters(self.h, other.h, int(num_actor_layers_to_share),
                                                  int(num_critic_layers_to_share)))
        other._share_keepalive = getattr(other, "_share_keepalive", []) + [self]

    def ShareReplayMemory(self, other):
        """src/dqn.cpp:1080-1082: `other` uses this learner's replay memory."""
        self._ck(self.lib.dqnhip_share_replay_memory(self.h, other.h))
        other._share_keepalive = getattr(other, "_share_keepalive", []) + [self]

    def debug_read(self, name):
        B = self.kMinibatchSize
        if name.startswith("act") and name[3:4].isdigit():      # "act<pass>_<layer>": stored tower activations [B][width]
            width = self.cfg.hidden[int(name.split("_")[1]) - 1]
            out = np.empty(B * width, np.float32)
            self._ck(self.lib.dqnhip_debug_read(self.h, name.encode(), _p(out), out.size))
            return out.reshape(B, width)
        if name.startswith("w16_"):       # "w16_<net>": the fp16 weight mirror of a net, widened, dense Caffe order like get_params
            out = np.empty(self.param_count(int(name[4:])), np.float32)
            self._ck(self.lib.dqnhip_debug_read(self.h, name.encode(), _p(out), out.size))
            return out
        if name in ("dz_c", "dz_a"):      # tower-top gradients [B][last hidden width] (fp16 learner: the scaled panel, widened)
            width = self.cfg.hidden[self.cfg.num_hidden - 1]
            out = np.empty(B * width, np.float32)
            self._ck(self.lib.dqnhip_debug_read(self.h, name.encode(), _p(out), out.size))
            return out.reshape(B, width)
        if name == "optimiser_launches":      # host counters [k_adam_soft*, k_solver_soft<>, k_solver_soft_gather<>], enqueued or captured
            out = np.zeros(3, np.float32)
            self._ck(self.lib.dqnhip_debug_read(self.h, name.encode(), _p(out), out.size))
            return out.astype(np.int64)
        if name == "sched_launches":          # ... and [k_sched_soft<>, k_sched_soft_gather<>]: the pass of a learner with an lr policy or a weight decay
            out = np.zeros(2, np.float32)
            self._ck(self.lib.dqnhip_debug_read(self.h, name.encode(), _p(out), out.size))
            return out.astype(np.int64)
        wide = name in ("actor_out", "dq_da", "actor_target_out", "dxc", "actor_target_smoothed", "target_noise_z")
        out = np.empty(B * (10 if wide else 1), np.float32)
        self._ck(self.lib.dqnhip_debug_read(self.h, name.encode(), _p(out), out.size))
        return out.reshape(B, 10) if wide else out

    def grad_buffer(self, net):
        ptr, n = C.c_void_p(), C.c_size_t()
        self._ck(self.lib.dqnhip_grad_buffer(self.h, net, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def stream(self):
        s = C.c_void_p()
        self._ck(self.lib.dqnhip_get_stream(self.h, C.byref(s)))
        return s.value

    def update_plan(self):
        """The launch plan of this learner's update (dqnhip_get_update_plan): the merged forms it takes, by name, and the kernels per
        update counted from a capture of the sequence dqnhip_update* enqueues."""
        p = capi.UpdatePlan()
        p.struct_size = C.sizeof(capi.UpdatePlan)
        self._ck(self.lib.dqnhip_get_update_plan(self.h, C.byref(p)))
        return {"forms": [n for i, n in enumerate(capi.PLAN_FORMS) if p.forms >> i & 1], "launches_single": p.launches_single,
                "launches_graph_first": p.launches_graph_first, "launches_in_graph": p.launches_in_graph,
                "updates_per_graph": p.updates_per_graph, "collectives": p.collectives, "solver": capi.SOLVERS[p.solver_type],
                "lr_policy": capi.LR_POLICIES[p.lr_policy], "regularised": bool(p.regularised)}

    # -- update diagnostics (include/dqnhip.h: Caffe's debug_info, reduced on the device; opt-in) --------------
    def diag_collect_raw(self):
        """dqnhip_diag_collect -> the ctypes report (capi.DiagReport)."""
        r = capi.DiagReport()
        r.struct_size = C.sizeof(capi.DiagReport)
        self._ck(self.lib.dqnhip_diag_collect(self.h, C.byref(r)))
        return r

    def diagnostics(self):
        """What the last update left on the device, as a plain dict (include/dqnhip.h has every definition):
        blobs   one dict per parameter blob in the dense Caffe order of get_params (actor, then critic): net, layer (the Caffe layer
                name), is_bias, count and the moments w / g / lag / step (dicts: count, n_zero, n_nonfinite, sum_abs, sum_sq,
                max_abs), g_hist (int32[64])
        panels  one dict per stored activation panel: pass, layer (1 .. L), rows, cols, the moments a, hist, n_negative, dead_units
        rows    q_target, y, q_train, q_policy, td (min, max, sum, sum_sq, n_nonfinite), n_terminal, actor_out (10 dicts), dq_da and,
                on a prioritized learner, per
        and the scalars: actor_iter, critic_iter, critic_loss, avg_q, grad_norm / clip_scale (by net), loss_scale (fp16 learner)."""
        r = self.diag_collect_raw()
        L = self.cfg.num_hidden

        def mom(m):
            return {"count": m.count, "n_zero": m.n_zero, "n_nonfinite": m.n_nonfinite, "sum_abs": m.sum_abs, "sum_sq": m.sum_sq,
                    "max_abs": m.max_abs}

        def name(b):
            if b.layer < L:
                return "ip%d_layer" % (b.layer + 1)
            if b.net == CRITIC:
                return "q_values_layer"
            return "action_layer" if b.layer == L else "actionpara_layer"

        blobs = [{"net": b.net, "layer": name(b), "is_bias": bool(b.is_bias), "count": b.w.count, "w": mom(b.w), "g": mom(b.g),
                  "lag": mom(b.lag), "step": mom(b.step), "g_hist": np.array(b.g_hist, np.int32)} for b in r.blobs[:r.n_blobs]]
        panels = [{"pass": p.pass_, "layer": p.layer, "rows": p.rows, "cols": p.cols, "a": mom(p.a), "hist": np.array(p.hist, np.int32),
                   "n_negative": p.n_negative, "dead_units": p.dead_units} for p in r.panels[:r.n_panels]]
        rows = {k: {"min": v.min, "max": v.max, "sum": v.sum, "sum_sq": v.sum_sq, "n_nonfinite": v.n_nonfinite}
                for k, v in (("q_target", r.q_target), ("y", r.y), ("q_train", r.q_train), ("q_policy", r.q_policy), ("td", r.td))}
        rows["n_terminal"] = r.n_terminal
        rows["actor_out"] = [{"min": a.min, "max": a.max, "sum": a.sum, "n_out_of_bounds": a.n_out_of_bounds} for a in r.actor_out]
        rows["dq_da"] = {"sum_abs": r.dq_da_sum_abs, "max_abs": r.dq_da_max_abs}
        rows["per"] = ({"w_min": r.per_w_min, "w_sum": r.per_w_sum, "prob_min": r.per_prob_min, "td_abs_max": r.per_td_abs_max}
                       if r.has_per else None)
        out = {"blobs": blobs, "panels": panels, "rows": rows, "has_per": bool(r.has_per), "actor_iter": r.actor_iter,
               "critic_iter": r.critic_iter, "critic_loss": r.critic_loss, "avg_q": r.avg_q,
               "grad_norm": {ACTOR: r.grad_norm[0], CRITIC: r.grad_norm[1]}, "clip_scale": {ACTOR: r.clip_scale[0], CRITIC: r.clip_scale[1]},
               "loss_scale": None}
        if r.fp16:
            out["loss_scale"] = {"mode": r.loss_scale_mode, "critic": r.loss_scale_critic, "dqda": r.loss_scale_dqda,
                                 "actor": r.loss_scale_actor, "mult_critic": r.mult_critic, "mult_actor": r.mult_actor}
        return out

    # -- prioritized replay (include/dqnhip.h: no reference counterpart, off unless enabled) -----------------
    def enable_prioritized_replay(self, alpha=None, beta0=None, beta_anneal_iters=None, eps=None, seed=None):
        """dqnhip_per_enable.  Arguments left None keep dqnhip_per_default_config's values: the customary ones of Schaul et al.
        2016, not measured on this workload."""
        c = capi.PerConfig()
        self.lib.dqnhip_per_default_config(C.byref(c))
        for name, v in (("alpha", alpha), ("beta0", beta0), ("beta_anneal_iters", beta_anneal_iters), ("eps", eps), ("seed", seed)):
            if v is not None:
                setattr(c, name, v)
        self._ck(self.lib.dqnhip_per_enable(self.h, C.byref(c)))

    def per_state(self):
        """dqnhip_per_get_state as a dict."""
        s = capi.PerState()
        s.struct_size = C.sizeof(capi.PerState)
        self._ck(self.lib.dqnhip_per_get_state(self.h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in capi.PerState._fields_ if name not in ("struct_size", "reserved")}

    def per_priorities(self, first, n):
        """the stored leaves (p^alpha) of the logical range [first, first + n)"""
        out = np.empty(int(n), np.float32)
        self._ck(self.lib.dqnhip_per_get_priorities(self.h, int(first), int(n), _p(out)))
        return out

    def set_per_priorities(self, first, p):
        a = _f32(p)
        self._ck(self.lib.dqnhip_per_set_priorities(self.h, int(first), a.size, _p(a)))

    def per_sample(self, counter, n_batches=1):
        """The sampler alone -> (idx [n_batches][B] int32, prob [n_batches][B] float32)."""
        B = self.kMinibatchSize
        idx, prob = np.empty((int(n_batches), B), np.int32), np.empty((int(n_batches), B), np.float32)
        self._ck(self.lib.dqnhip_per_sample(self.h, int(counter), int(n_batches), idx.ctypes.data_as(capi.ip), _p(prob)))
        return idx, prob

    def per_debug_read(self, name):
        """"level<k>" (every real node of the level) or one of "u", "slot", "prob", "w", "td_abs" ([B], "slot" as int64)."""
        if name.startswith("level"):
            n = self.cfg.replay_capacity
            for _ in range(int(name[5:])):
                n = (n + 63) // 64
        else:
            n = self.kMinibatchSize
        out = np.empty(n, np.float32)
        self._ck(self.lib.dqnhip_per_debug_read(self.h, name.encode(), _p(out), out.size))
        return out.astype(np.int64) if name == "slot" else out

    # -- n-step returns (include/dqnhip.h: no reference counterpart, off unless enabled) ----------------------
    def enable_n_step(self, n):
        """dqnhip_nstep_enable: the off-policy target becomes sum_{k<m} gamma^k r_{t+k} + gamma^m Q'(s_{t+m}, mu'(s_{t+m})) with m <= n
        (shorter at a terminal transition and at the memory's end).  n in 1 .. 64 (1: the 1-step learner's bits, on the n-step
        schedule); may be called again; there is no disable.  Typical n (3 - 5) is the literature's value, not measured here."""
        self._ck(self.lib.dqnhip_nstep_enable(self.h, int(n)))

    def enable_target_smoothing(self, sigma_logits=None, sigma_params=None, clip=None, clamp=None, seed=None):
        """Target policy smoothing (TD3; include/dqnhip.h): the critic-target sees clamp(mu'(s') + range clip(sigma z, -clip, clip)).
        Sigmas and clip in units of each column's range; what is left None keeps the default (sigma 0.1, clip 0.25, clamp on: TD3's
        values on a range of 2, not measured on this workload)."""
        cfg = capi.NoiseConfig()
        self._ck(self.lib.dqnhip_noise_default_config(C.byref(cfg), capi.NOISE_TARGET))
        for k, v in (("sigma_logits", sigma_logits), ("sigma_params", sigma_params), ("clip", clip), ("seed", seed)):
            if v is not None:
                setattr(cfg, k, v)
        if clamp is not None:
            cfg.clamp = 1 if clamp else 0
        self._ck(self.lib.dqnhip_target_noise_enable(self.h, C.byref(cfg)))

    def target_smoothing(self):
        """None while target smoothing is off, else its config as a dict."""
        on, cfg = C.c_int32(), capi.NoiseConfig()
        self._ck(self.lib.dqnhip_target_noise_get(self.h, C.byref(on), C.byref(cfg)))
        if not on.value:
            return None
        return dict(sigma_logits=cfg.sigma_logits, sigma_params=cfg.sigma_params, clip=cfg.clip, clamp=bool(cfg.clamp), seed=cfg.seed)

    def target_noise_counter(self):
        """The Philox counter the last update's target noise was keyed by (debug_read "target_noise_counter")."""
        out = np.empty(2, np.float32)
        self._ck(self.lib.dqnhip_debug_read(self.h, b"target_noise_counter", _p(out), 2))
        return int(out[0]) + (int(out[1]) << 24)

    def n_step(self):
        """dqnhip_nstep_get: n, or 0 if n-step returns were never enabled."""
        n = C.c_int32()
        self._ck(self.lib.dqnhip_nstep_get(self.h, C.byref(n)))
        return n.value

    def n_step_debug_read(self, name):
        """Of the last update, [B]: "reward" (the window's discounted reward sum, float32), "steps" (the window's length, int64) or
        "disc" (gamma^steps, float64)."""
        B = self.kMinibatchSize
        if name == "disc":
            out = np.empty(B, np.float64)
            self._ck(self.lib.dqnhip_nstep_debug_read_f64(self.h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
            return out
        out = np.empty(B, np.float32)
        self._ck(self.lib.dqnhip_nstep_debug_read(self.h, name.encode(), _p(out), out.size))
        return out.astype(np.int64) if name == "steps" else out

    def validate_memory(self, first=0, n=None):
        """dqnhip_nstep_validate over the logical transitions [first, first + n) (n = None: to the end) -> (violations, first_bad):
        how many non-terminal transitions' stored next state is not, bit for bit, the state of their logical successor, and the
        smallest such index (-1: none).  Any learner may validate."""
        v, fb = C.c_int64(), C.c_int32()
        self._ck(self.lib.dqnhip_nstep_validate(self.h, int(first), -1 if n is None else int(n), C.byref(v), C.byref(fb)))
        return v.value, fb.value

    # -- replay sweep (include/dqnhip.h: the nets evaluated over the stored memory, opt-in) -------------------
    @staticmethod
    def _sweep_dict(r):
        out = {k: {"min": v.min, "max": v.max, "sum": v.sum, "sum_sq": v.sum_sq, "n_nonfinite": v.n_nonfinite}
               for k, v in (("q", r.q), ("y", r.y), ("td", r.td), ("q_policy", r.q_policy), ("mc", r.mc), ("q_minus_mc", r.q_minus_mc),
                            ("reward", r.reward))}
        out.update({"first": r.first, "n": r.n, "n_chunks": r.n_chunks, "n_terminal": r.n_terminal, "n_action_match": r.n_action_match,
                    "td_hist": np.array(r.td_hist, np.int32), "actor_iter": r.actor_iter, "critic_iter": r.critic_iter})
        return out

    def evaluate_memory_raw(self, first=0, n=-1, rows=None):
        """dqnhip_evaluate_memory -> the ctypes report (capi.SweepReport); rows: a capi.SweepRows or None."""
        r = capi.SweepReport()
        r.struct_size = C.sizeof(capi.SweepReport)
        self._ck(self.lib.dqnhip_evaluate_memory(self.h, int(first), int(n), C.byref(r), C.byref(rows) if rows is not None else None))
        return r

    def evaluate_memory(self, first=0, n=-1, rows=False):
        """The nets as they stand evaluated over the logical transitions [first, first + n) (n = -1: to the end of the memory), as a
        plain dict shaped like diagnostics()'s rows: q, y, td, q_policy, mc, q_minus_mc, reward (min, max, sum, sum_sq, n_nonfinite),
        n, n_chunks, n_terminal, n_action_match, td_hist (int32[64]), actor_iter, critic_iter.  rows=True adds "rows": the per-transition
        arrays q, y, td, q_policy (float32[n]) and action_match (int32[n]).  Overwrites what debug_read / diagnostics read."""
        if not rows:
            return self._sweep_dict(self.evaluate_memory_raw(first, n))
        count = self.memory_size() - int(first) if int(n) < 0 else int(n)
        arr = {k: np.zeros(max(count, 0), np.float32) for k in ("q", "y", "td", "q_policy")}
        arr["action_match"] = np.zeros(max(count, 0), np.int32)
        sr = capi.SweepRows()
        sr.struct_size = C.sizeof(capi.SweepRows)
        for k in ("q", "y", "td", "q_policy"):
            setattr(sr, k, _p(arr[k]))
        sr.action_match = arr["action_match"].ctypes.data_as(capi.ip)
        # (the count the arrays were sized for, never -1: a shared ring may have grown since memory_size() was read)
        out = self._sweep_dict(self.evaluate_memory_raw(first, n if int(n) >= 0 or count < 0 else count, sr))      # (count < 0: first lies outside, refused)
        out["rows"] = arr
        return out

    def per_refresh(self, first=0, n=-1):
        """dqnhip_per_refresh: the sweep of evaluate_memory on a prioritized learner, every leaf of the window rewritten to
        (|td| + eps)^alpha.  Returns evaluate_memory's dict."""
        r = capi.SweepReport()
        r.struct_size = C.sizeof(capi.SweepReport)
        self._ck(self.lib.dqnhip_per_refresh(self.h, int(first), int(n), C.byref(r)))
        return self._sweep_dict(r)

    # -- native learner-state file (include/dqnhip.h: exact resume, opt-in) ----------------------------------
    def save_state(self, path, memory=True, user=b"", wait=True):
        """dqnhip_save_state: everything a bit-exact resume needs, in one file; `user` is an opaque section of the caller's.
        wait=False: dqnhip_save_state_async — the same bytes, frozen on the device at this point of the stream and written by the
        learner's writer thread while training goes on; save_state_wait() joins it and reports its status."""
        user = bytes(user)
        fn = self.lib.dqnhip_save_state if wait else self.lib.dqnhip_save_state_async
        self._ck(fn(self.h, os.fsencode(path), 0 if memory else capi.STATE_NO_MEMORY, user or None, len(user)))

    def save_state_wait(self):
        """dqnhip_save_state_wait: joins an asynchronous save in flight; raises if it failed."""
        self._ck(self.lib.dqnhip_save_state_wait(self.h))

    def save_state_done(self):
        """dqnhip_save_state_poll: True when no asynchronous save is in flight.  Never blocks."""
        done = C.c_int32()
        self._ck(self.lib.dqnhip_save_state_poll(self.h, C.byref(done)))
        return bool(done.value)

    def state_crc32_device(self, data, misalign=0):
        """dqnhip_state_crc32_device: the asynchronous save's checksum path on `data` (bytes); equals zlib.crc32(data)."""
        data = bytes(data)
        crc = C.c_uint32()
        self._ck(self.lib.dqnhip_state_crc32_device(self.h, data or None, len(data), int(misalign), C.byref(crc)))
        return crc.value

    def load_state(self, path):
        """dqnhip_load_state: validates the whole file first; a failure leaves the learner untouched."""
        self._ck(self.lib.dqnhip_load_state(self.h, os.fsencode(path)))
        self.cfg.seed = state_info(path)["seed"]        # the learner adopted the file's sampling key

    def set_kernel_timing(self, enable):
        self._ck(self.lib.dqnhip_set_kernel_timing(self.h, int(enable)))

    def kernel_timing(self, family, reset=False):
        ms, n = C.c_float(), C.c_int64()
        self._ck(self.lib.dqnhip_get_kernel_timing(self.h, family.encode(), C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value


def FindLatestSnapshot(snapshot_prefix):
    """src/dqn.cpp:122-144 -> (actor_solverstate, critic_solverstate, replaymemory), '' if none."""
    lib = capi.load()
    bufs = [C.create_string_buffer(4096) for _ in range(3)]
    if lib.dqnhip_find_latest_snapshot(os.fsencode(snapshot_prefix), bufs[0], bufs[1], bufs[2], 4096) != 0:
        raise DQNFatal(lib.dqnhip_last_error().decode())
    return tuple(os.fsdecode(b.value) for b in bufs)


def state_info(path):
    """dqnhip_state_info as a dict (no GPU needed): validates the whole file and reports its header."""
    lib = capi.load()
    s = capi.StateInfo()
    s.struct_size = C.sizeof(capi.StateInfo)
    if lib.dqnhip_state_info(os.fsencode(path), C.byref(s)) != 0:
        raise DQNFatal(lib.dqnhip_last_error().decode())
    d = {name: getattr(s, name) for name, _ in capi.StateInfo._fields_ if name not in ("struct_size", "hidden")}
    d["hidden"] = tuple(s.hidden[i] for i in range(max(0, min(s.num_hidden, capi.MAX_HIDDEN))))
    return d


def state_user(path):
    """dqnhip_state_read_user: the caller's section of a learner-state file as bytes (no GPU needed)."""
    lib = capi.load()
    n = C.c_size_t()
    cap = max(1, state_info(path)["user_bytes"])
    buf = C.create_string_buffer(cap)
    if lib.dqnhip_state_read_user(os.fsencode(path), buf, cap, C.byref(n)) != 0:
        raise DQNFatal(lib.dqnhip_last_error().decode())
    return buf.raw[:n.value]


def FindHiScore(snapshot_prefix):
    """src/dqn.cpp:146-158."""
    lib = capi.load()
    v = C.c_int32()
    if lib.dqnhip_find_hiscore(os.fsencode(snapshot_prefix), C.byref(v)) != 0:
        raise DQNFatal(lib.dqnhip_last_error().decode())
    return v.value


def RemoveFilesMatchingRegexp(regexp):
    """src/dqn.cpp:92-98."""
    lib = capi.load()
    if lib.dqnhip_remove_files_matching_regexp(os.fsencode(regexp)) != 0:
        raise DQNFatal(lib.dqnhip_last_error().decode())


def FilesMatchingRegexp(regexp):
    """src/dqn.hpp:213-216: regular files in the regexp's directory whose name matches its last component."""
    lib = capi.load()
    n = C.c_int32()
    size = 1 << 16
    while True:
        buf = C.create_string_buffer(size)
        if lib.dqnhip_files_matching_regexp(os.fsencode(regexp), buf, size, C.byref(n)) == 0:
            return [os.fsdecode(x) for x in buf.value.split(b"\n") if x]
        msg = lib.dqnhip_last_error().decode()
        if "buffer too small" not in msg or size > (1 << 26):
            raise DQNFatal(msg)
        size *= 4


def RemoveSnapshots(regexp, min_iter):
    """src/dqn.hpp:222-224, src/dqn.cpp:100-109."""
    lib = capi.load()
    if lib.dqnhip_remove_snapshots(os.fsencode(regexp), int(min_iter)) != 0:
        raise DQNFatal(lib.dqnhip_last_error().decode())


def dp_rendezvous_file(path, rank, world, unique_id=None, timeout_s=120):
    """File rendezvous of a data-parallel group (needs no GPU): rank 0 passes the id, the others receive it."""
    lib = capi.load()
    buf = C.create_string_buffer(bytes(unique_id) if unique_id is not None else b"", capi.DP_ID_BYTES)
    if lib.dqnhip_dp_rendezvous_file(os.fsencode(path), int(rank), int(world), int(timeout_s), buf, capi.DP_ID_BYTES) != 0:
        raise DQNFatal(lib.dqnhip_last_error().decode())
    return buf.raw


def dp_rendezvous_cleanup(path, world):
    capi.load().dqnhip_dp_rendezvous_cleanup(os.fsencode(path), int(world))


def reduce_gradients_local(learners, net):
    """Sum the gradient arenas of co-located learners of one data-parallel group (rank order)."""
    lib = capi.load()
    arr = (capi.H * len(learners))(*[l.h for l in learners])
    if lib.dqnhip_reduce_gradients_local(arr, len(learners), net) != 0:
        raise DQNFatal(lib.dqnhip_last_error().decode())


class EnvFrontEnd:
    """N concurrent (synthetic) HFO workers feeding one learner's device-resident replay:
    the learner side of PlayOneEpisode (src/dqn_main.cpp:97-153), batched.  See
    include/dqnhip_env.h."""

    def __init__(self, dqn, workers, max_steps=500, unum=7, p_end=0.01, p_goal=0.3, seed=1):
        self.dqn, self.N = dqn, workers
        self.lib = dqn.lib
        cfg = capi.EnvConfig()
        cfg.struct_size = C.sizeof(capi.EnvConfig)
        cfg.workers, cfg.max_steps, cfg.unum = workers, max_steps, unum
        cfg.p_end, cfg.p_goal, cfg.seed = p_end, p_goal, seed
        self.h = C.c_void_p()
        dqn._ck(self.lib.dqnhip_env_create(dqn.h, C.byref(cfg), C.byref(self.h)))

    def step(self, epsilon, n_steps=1):
        self.dqn._ck(self.lib.dqnhip_env_step(self.h, float(epsilon), int(n_steps)))

    def stats(self):
        a, b, g = C.c_int64(), C.c_int64(), C.c_int64()
        r = C.c_double()
        self.dqn._ck(self.lib.dqnhip_env_stats(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(g)))
        return a.value, b.value, r.value, g.value

    def debug_read(self, name):
        N, S = self.N, self.dqn.state_size_
        if name == "truncated":
            out = np.empty(1, np.float32)
            self.dqn._ck(self.lib.dqnhip_env_debug_read(self.h, name.encode(), _p(out), 1))
            return int(out[0])
        if name == "graph_nodes":
            out = np.empty(2, np.float32)
            self.dqn._ck(self.lib.dqnhip_env_debug_read(self.h, name.encode(), _p(out), 2))
            return int(out[0]), int(out[1])
        rows10 = name in ("actor_out", "greedy_out", "noise_state", "noise_z")
        n = N * (S if name == "state" else 10 if rows10 else 1)
        out = np.empty(n, np.float32)
        self.dqn._ck(self.lib.dqnhip_env_debug_read(self.h, name.encode(), _p(out), n))
        if name == "state":
            return out.reshape(N, S)
        if rows10:
            return out.reshape(N, 10)
        return out

    def set_noise(self, enable=True, sigma_logits=None, sigma_params=None, theta=None, clamp=None, seed=None):
        """Exploration noise on the greedy ActorOutput, on the device (include/dqnhip_env.h): an Ornstein-Uhlenbeck state per worker
        and column, theta = 1 for white Gaussian noise; sigmas in units of the column's range.  What is left None keeps the
        default (theta 0.15, sigma_params 0.1, sigma_logits 0, clamp on: the literature's values, not measured on this workload).
        set_noise(False) switches it off.  Every call zeroes the OU states."""
        if not enable:
            self.dqn._ck(self.lib.dqnhip_env_set_noise(self.h, None))
            return
        cfg = capi.NoiseConfig()
        self.dqn._ck(self.lib.dqnhip_noise_default_config(C.byref(cfg), capi.NOISE_EXPLORE))
        for k, v in (("sigma_logits", sigma_logits), ("sigma_params", sigma_params), ("theta", theta), ("seed", seed)):
            if v is not None:
                setattr(cfg, k, v)
        if clamp is not None:
            cfg.clamp = 1 if clamp else 0
        self.dqn._ck(self.lib.dqnhip_env_set_noise(self.h, C.byref(cfg)))

    def close(self):
        if self.h:
            self.lib.dqnhip_env_destroy(self.h)
            self.h = None


EnvEpisode = namedtuple("EnvEpisode", "total_reward extrinsic_reward steps status worker step_index")


class ExternalEnv(EnvFrontEnd):
    """N concurrent HFO workers whose states the caller supplies (a rack of HFO servers, any batched simulator that emits HFO
    low-level features): `act` is the batched step up to GetAction, `observe` takes what the simulator answered and does the rest
    of PlayOneEpisode's learner side on the device.  record=False plays PlayOneEpisode(update = false), the mode of Evaluate()
    (src/dqn_main.cpp:171-204): nothing reaches the replay memory.  See include/dqnhip_env.h."""

    def __init__(self, dqn, workers, first_states, max_steps=500, unum=7, seed=1, record=True):
        self.dqn, self.N = dqn, workers
        self.lib = dqn.lib
        cfg = capi.EnvConfig()
        cfg.struct_size = C.sizeof(capi.EnvConfig)
        cfg.workers, cfg.max_steps, cfg.unum, cfg.seed = workers, max_steps, unum, seed
        first = _f32(first_states)
        if first.shape != (workers, dqn.state_size_):
            raise ValueError("first_states must be [workers, state_size]")
        self.h = C.c_void_p()
        dqn._ck(self.lib.dqnhip_env_create_external(dqn.h, C.byref(cfg), 0 if record else capi.ENV_NO_RECORD, _p(first), C.byref(self.h)))

    def step(self, epsilon, n_steps=1):
        self.dqn._ck(self.lib.dqnhip_env_step(self.h, float(epsilon), int(n_steps)))      # refused: names act / observe

    def act(self, epsilon, actor_out=False):
        """-> (action [N] int32, args [N,2]) and, with actor_out=True, the chosen ActorOutputs [N,10]."""
        action, args = np.empty(self.N, np.int32), np.empty((self.N, 2), np.float32)
        ao = np.empty((self.N, 10), np.float32) if actor_out else None
        self.dqn._ck(self.lib.dqnhip_env_act(self.h, float(epsilon), action.ctypes.data_as(capi.ip), _p(args), _p(ao) if actor_out else None))
        return (action, args, ao) if actor_out else (action, args)

    def observe(self, next_states, status, player_on_ball):
        nx = _f32(next_states)
        st, pob = np.ascontiguousarray(status, np.int32), np.ascontiguousarray(player_on_ball, np.int32)
        if nx.shape != (self.N, self.dqn.state_size_) or st.shape != (self.N,) or pob.shape != (self.N,):
            raise ValueError("observe takes next_states [workers, state_size], status [workers], player_on_ball [workers]")
        self.dqn._ck(self.lib.dqnhip_env_observe(self.h, _p(nx), st.ctypes.data_as(capi.ip), pob.ctypes.data_as(capi.ip)))

    def act_device(self, epsilon, action_ptr, args_ptr, actor_out_ptr=None):
        """Device pointers (ints): int32 [N], float [N,2], float [N,10] or None.  Asynchronous on the learner's stream."""
        self.dqn._ck(self.lib.dqnhip_env_act_device(self.h, float(epsilon), action_ptr, args_ptr, actor_out_ptr))

    def observe_device(self, next_states_ptr, status_ptr, player_on_ball_ptr):
        """Device pointers (ints): float [N,S] dense, int32 [N], int32 [N].  Asynchronous on the learner's stream."""
        self.dqn._ck(self.lib.dqnhip_env_observe_device(self.h, next_states_ptr, status_ptr, player_on_ball_ptr))

    def episodes(self, cap=None):
        """The finished episodes not handed out yet (at most `cap`), in (step_index, worker) order; also sets self.dropped."""
        out = []
        while cap is None or len(out) < cap:
            want = 256 if cap is None else min(256, cap - len(out))
            buf = (capi.EnvEpisode * want)()
            n, dropped = C.c_int32(), C.c_int64()
            self.dqn._ck(self.lib.dqnhip_env_read_episodes(self.h, buf, want, C.byref(n), C.byref(dropped)))
            self.dropped = dropped.value
            out += [EnvEpisode(r.total_reward, r.extrinsic_reward, r.steps, r.status, r.worker, r.step_index) for r in buf[:n.value]]
            if n.value < want:
                break
        return out


def get_avg_std(values):
    """src/dqn_main.cpp:155-166: the mean and the standard deviation with the n - 1 divisor (nan where the reference divides 0 by 0)."""
    v = np.asarray(list(values), np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.float64(v.sum()) / np.float64(v.size)
        std = np.sqrt(np.float64(((v - avg) ** 2).sum()) / np.float64(v.size - 1.0))
    return float(avg), float(std)


def evaluation_summary(episodes):
    """The fields of Evaluate()'s log line (src/dqn_main.cpp:171-204) from finished episodes (ExternalEnv.episodes(), or anything
    with total_reward / steps / status): a trial is successful when its status is GOAL (1); goal_perc is the function's result."""
    eps = list(episodes)
    if not eps:
        raise ValueError("evaluation_summary needs at least one episode")
    avg_reward, reward_std = get_avg_std(e.total_reward for e in eps)
    avg_steps, steps_std = get_avg_std(e.steps for e in eps)
    success_steps, success_std = get_avg_std(e.steps for e in eps if e.status == 1)
    goals = sum(1 for e in eps if e.status == 1)
    return dict(episodes=len(eps), avg_reward=avg_reward, reward_std=reward_std, avg_steps=avg_steps, steps_std=steps_std,
                success_steps=success_steps, success_std=success_std, goals=goals, goal_perc=float(np.float32(goals) / np.float32(len(eps))))
