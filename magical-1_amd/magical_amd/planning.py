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
