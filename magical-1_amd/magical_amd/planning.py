"""Planners on the simulator's plan() (mg_plan: K candidate rollouts per env, best-of-K chosen on the device).

`ShootingPolicy` is random shooting, the simplest model-predictive controller: at every decision it draws K random
action sequences of H env-steps per env (sample_plans), rolls all of them out from the envs' current states without
touching them (plan), and plays the first action of each env's best sequence.  The candidates come from the device
generator, so a run is a function of (key, the envs' states) alone.

Every planner takes an `Objective`: what a rollout is worth.  The default, the score of the rollout's final state, is
blind to a goal that was crossed and left again and ignores the env's dense reward; `Objective("return")` is the
discounted sum of the rewards step() would pay over the horizon (plus `tail` times the discounted final score when the
episode goes on past it), `Objective("peak")` the best discounted score at any step of the horizon.
"""
import math

OBJECTIVE_KINDS = {"final": 0, "return": 1, "peak": 2}   # MG_OBJ_* (include/magical_sim.h)


class Objective:
    """What a rollout is worth (mg_objective): kind 'final' (the final state's score s_n), 'return' (sum over the
    simulated steps k of gamma^(k-1) * reward_k, plus tail * gamma^n * s_n unless the episode ended inside the horizon)
    or 'peak' (max over k of gamma^k * s_k, the entry state included).  gamma in (0, 1]; tail finite and >= 0.  An
    immutable value: equal fields compare equal."""

    __slots__ = ("kind", "gamma", "tail")

    def __init__(self, kind="final", gamma=1.0, tail=0.0):
        if kind not in OBJECTIVE_KINDS:
            raise ValueError(f"Objective: kind must be one of {sorted(OBJECTIVE_KINDS)}, got {kind!r}")
        try:
            gamma, tail = float(gamma), float(tail)
        except (TypeError, ValueError):
            raise ValueError("Objective: gamma and tail must be numbers") from None
        if not 0.0 < gamma <= 1.0:
            raise ValueError(f"Objective: gamma must be in (0, 1], got {gamma}")
        if not (math.isfinite(tail) and tail >= 0.0):
            raise ValueError(f"Objective: tail must be finite and not negative, got {tail}")
        object.__setattr__(self, "kind", kind)
        object.__setattr__(self, "gamma", gamma)
        object.__setattr__(self, "tail", tail)

    def __setattr__(self, name, value):
        raise AttributeError("Objective is immutable")

    @property
    def kind_id(self):
        return OBJECTIVE_KINDS[self.kind]

    def _key(self):
        return (self.kind, self.gamma, self.tail)

    def __eq__(self, other):
        return isinstance(other, Objective) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"Objective(kind={self.kind!r}, gamma={self.gamma!r}, tail={self.tail!r})"


def as_objective(objective, fn):
    """None or an Objective, for the `objective=` argument of fn; anything else is a ValueError (a kind name is
    accepted as shorthand for Objective(kind))."""
    if objective is None or isinstance(objective, Objective):
        return objective
    if isinstance(objective, str):
        return Objective(objective)
    raise ValueError(f"{fn}: objective must be None, a kind name or a magical_amd.Objective, got {type(objective).__name__}")


def plan_step(t, horizon, candidates, repeat=1):
    """The generator counter decision t starts from: a decision draws `candidates` sequences of ceil(horizon /
    repeat) held actions and consumes as many counter values (mg_plan_sample), so decisions never share any."""
    return int(t) * int(candidates) * -(-int(horizon) // int(repeat))


def cem_step(t, horizon, candidates, iters, repeat=1):
    """The generator counter CEM decision t starts from: a decision runs `iters` rounds of `candidates` sequences of
    ceil(horizon / repeat) held actions and consumes as many counter values (mg_plan_cem)."""
    return int(t) * int(iters) * int(candidates) * -(-int(horizon) // int(repeat))


def shift_weights(weights):
    """CEM weights u16[J, 18, N] moved one slot towards the present: slot j <- slot j + 1, the last slot all ones (a
    new tensor)."""
    import torch
    w = weights.view(torch.int16)
    return torch.cat([w[1:], torch.ones_like(w[:1])]).view(torch.uint16)


class CEMPolicy:
    """policy(obs) -> uint8 actions [N], ShootingPolicy's contract with the cross-entropy method in place of one round
    of uniform candidates: every decision is one plan_cem() of `iters` rounds of `candidates` sequences of `horizon`
    env-steps, refitted to the `elites` best with smoothing count `alpha`, and plays the first action of each env's
    best sequence.  Decision t draws from counter cem_step(t, ...) on.  warm_start=True (repeat == 1 only: a slot is
    then one env-step) carries the fitted weights to the next decision, shifted one slot towards the present with the
    last slot reset to all ones; reset() drops them and starts the decision counter again.  objective: the Objective
    the candidates are ranked by (None: the final state's score, plan_cem() as it always was)."""

    def __init__(self, env, horizon, candidates, iters, elites, alpha=1, repeat=1, key=42, warm_start=False,
                 objective=None):
        if int(horizon) < 1 or int(candidates) < 1 or int(iters) < 1 or int(repeat) < 1:
            raise ValueError("CEMPolicy: horizon, candidates, iters and repeat must be at least 1")
        if not 1 <= int(elites) <= int(candidates):
            raise ValueError("CEMPolicy: elites must be in [1, candidates]")
        if int(alpha) < 0:
            raise ValueError("CEMPolicy: alpha must not be negative")
        if warm_start and int(repeat) != 1:
            raise ValueError("CEMPolicy: warm_start needs repeat == 1 (the weights are shifted by one env-step)")
        self.env, self.horizon, self.candidates, self.iters = env, int(horizon), int(candidates), int(iters)
        self.elites, self.alpha, self.repeat, self.key, self.warm_start = int(elites), int(alpha), int(repeat), key, bool(warm_start)
        self.objective = as_objective(objective, "CEMPolicy")
        self.t = 0
        self.weights = None   # warm_start: the next decision's starting weights
        self.last = None      # the latest decision's plan_cem() result

    def reset(self):
        self.t = 0
        self.weights = None

    def __call__(self, obs=None):
        kw = {} if self.objective is None else {"objective": self.objective}
        self.last = self.env.plan_cem(self.horizon, self.candidates, self.iters, self.elites, alpha=self.alpha,
                                      repeat=self.repeat, key=self.key, weights=self.weights,
                                      step=cem_step(self.t, self.horizon, self.candidates, self.iters, self.repeat), **kw)
        if self.warm_start:
            self.weights = shift_weights(self.last["weights"])
        self.t += 1
        return self.last["first_action"]


class ShootingPolicy:
    """policy(obs) -> uint8 actions [N] for the env it was given (a VecMagicalEnv or PipelinedVecEnv): the first
    action of the best of `candidates` random sequences of `horizon` env-steps, each action held for `repeat` steps.
    The observation is not used -- the plan starts from the env's state -- so the policy fits
    BatchedEvaluationProtocol's policy(obs_dict) contract when it wraps the env being evaluated, and a plain
    reset() / step() loop.  reset() starts the decision counter again: two runs with the same key over the same env
    states give the same actions.  objective: the Objective the candidates are ranked by (None: the final state's
    score, plan() as it always was)."""

    def __init__(self, env, horizon, candidates, repeat=1, key=42, objective=None):
        if int(horizon) < 1 or int(candidates) < 1 or int(repeat) < 1:
            raise ValueError("ShootingPolicy: horizon, candidates and repeat must be at least 1")
        self.env, self.horizon, self.candidates, self.repeat, self.key = env, int(horizon), int(candidates), int(repeat), key
        self.objective = as_objective(objective, "ShootingPolicy")
        self.t = 0
        self.last = None   # the latest decision's plan() result

    def reset(self):
        self.t = 0

    def __call__(self, obs=None):
        acts = self.env.sample_plans(self.horizon, self.candidates, self.repeat, self.key,
                                     step=plan_step(self.t, self.horizon, self.candidates, self.repeat))
        self.last = self.env.plan(acts) if self.objective is None else self.env.plan(acts, objective=self.objective)
        self.t += 1
        return self.last["first_action"]


class BeamPolicy:
    """policy(obs) -> uint8 actions [N], ShootingPolicy's contract with beam search in place of whole-horizon rollouts:
    every decision draws `candidates` random sequences of `horizon` env-steps per env (sample_plans, counters as
    ShootingPolicy's: decision t draws from plan_step(t, ...) on), runs plan_beam() on them -- after every `seg`
    env-steps each env keeps its `survivors` best partial rollouts and refills the other slots with copies of them --
    and plays the first action of each env's best lineage.  objective: the Objective the slots are ranked by (None: the
    score of the state they have reached)."""

    def __init__(self, env, horizon, candidates, seg, survivors, repeat=1, key=42, objective=None):
        if int(horizon) < 1 or int(candidates) < 1 or int(repeat) < 1:
            raise ValueError("BeamPolicy: horizon, candidates and repeat must be at least 1")
        if not 1 <= int(seg) <= int(horizon):
            raise ValueError("BeamPolicy: seg must be in [1, horizon]")
        if not 1 <= int(survivors) <= int(candidates):
            raise ValueError("BeamPolicy: survivors must be in [1, candidates]")
        self.env, self.horizon, self.candidates, self.repeat, self.key = env, int(horizon), int(candidates), int(repeat), key
        self.seg, self.survivors = int(seg), int(survivors)
        self.objective = as_objective(objective, "BeamPolicy")
        self.t = 0
        self.last = None   # the latest decision's plan_beam() result

    def reset(self):
        self.t = 0

    def __call__(self, obs=None):
        acts = self.env.sample_plans(self.horizon, self.candidates, self.repeat, self.key,
                                     step=plan_step(self.t, self.horizon, self.candidates, self.repeat))
        kw = {} if self.objective is None else {"objective": self.objective}
        self.last = self.env.plan_beam(acts, self.seg, self.survivors, **kw)
        self.t += 1
        return self.last["first_action"]
