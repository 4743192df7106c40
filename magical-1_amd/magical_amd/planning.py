"""Planners on the simulator's plan() (mg_plan: K candidate rollouts per env, best-of-K chosen on the device).

`ShootingPolicy` is random shooting, the simplest model-predictive controller: at every decision it draws K random
action sequences of H env-steps per env (sample_plans), rolls all of them out from the envs' current states without
touching them (plan), and plays the first action of each env's best sequence.  The candidates come from the device
generator, so a run is a function of (key, the envs' states) alone.
"""


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
    last slot reset to all ones; reset() drops them and starts the decision counter again."""

    def __init__(self, env, horizon, candidates, iters, elites, alpha=1, repeat=1, key=42, warm_start=False):
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
        self.t = 0
        self.weights = None   # warm_start: the next decision's starting weights
        self.last = None      # the latest decision's plan_cem() result

    def reset(self):
        self.t = 0
        self.weights = None

    def __call__(self, obs=None):
        self.last = self.env.plan_cem(self.horizon, self.candidates, self.iters, self.elites, alpha=self.alpha,
                                      repeat=self.repeat, key=self.key, weights=self.weights,
                                      step=cem_step(self.t, self.horizon, self.candidates, self.iters, self.repeat))
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
    states give the same actions."""

    def __init__(self, env, horizon, candidates, repeat=1, key=42):
        if int(horizon) < 1 or int(candidates) < 1 or int(repeat) < 1:
            raise ValueError("ShootingPolicy: horizon, candidates and repeat must be at least 1")
        self.env, self.horizon, self.candidates, self.repeat, self.key = env, int(horizon), int(candidates), int(repeat), key
        self.t = 0
        self.last = None   # the latest decision's plan() result

    def reset(self):
        self.t = 0

    def __call__(self, obs=None):
        acts = self.env.sample_plans(self.horizon, self.candidates, self.repeat, self.key,
                                     step=plan_step(self.t, self.horizon, self.candidates, self.repeat))
        self.last = self.env.plan(acts)
        self.t += 1
        return self.last["first_action"]
