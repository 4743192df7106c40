"""The per-env MT19937 stream past its twists, in every reset path, against numpy's own RandomState.

Every env draws its layouts from a numpy-legacy MT19937 (mt_key [624][N], mt_pos [N]) that regenerates its 624 words
(the "twist") whenever pos reaches 624.  csrc/mg_reset.h twists in three ways -- serially over HBM (the auto-reset
fused into the robot scenes' step kernels, one diverged lane), cooperatively over the LDS copy with 64 lanes
(reset_kernel: reset(), masked resets, own-launch auto-resets, the next-layout shadow) and serially over the LDS copy
under a partial exec mask -- and a wrong index in any of them changes every layout from some episode on and nothing
else.  The reference is numpy: words are np.frombuffer(RandomState(seed).bytes(4 * k), "<u4"), states are
get_state()[1:3], every comparison is exact.

CPU tests pin the oracle (oracle/rng.c, and the oracle env's draws per reset) to numpy across several twists, and say
what the GPU cases below rely on: the words each variant draws per reset and the resets its twists fall in.

    variant                     words/reset   resets with a twist (after the first reset's)
    MoveToRegion-TestDynamics   10            63, 125          (both inside the reset)
    MoveToCorner-TestDynamics   14            45, 90           (both inside the reset)
    MoveToCorner-TestColour     5             125, 250         (inside; reset 250 starts at the odd pos 621, so the
    MoveToCorner-TestShape      5             125, 250          two words of its second double straddle the twist)
    MoveToCorner-Demo           4             157              (on the reset's first draw: 156 * 4 = 624)

GPU tests: LoRes4E sims, env i seeded 9100 + i, random actions from RandomState(7).  After every step the rng_state()
of ALL envs is compared with the reference stream, and the observations of envs 0, n // 2 and n - 1 with oracle envs
that are only reset() (a reset does not depend on the physics).  With max_episode_steps=1 every step ends in a reset.
MoveToCorner-Demo's run of 160 steps holds the one twist its row names (reset 157); every other run holds at least two
twists after the first reset's.

The explicit-reset case (PickAndPlace-Demo, 45 reset(mask) calls) rotates its two mask patterns with the call index
c: even calls reset the envs with (e + c // 2) % 2 == 1, odd calls those with (e + c // 2) % 3 == 0.  Fixed patterns
e % 2 / e % 3 == 0 would never reset envs 2 and 4 again; rotated, every env resets 18 to 20 times at its own pos.  At
about 50 words per reset that is two to three twists per env, the first reset's included, which is what the oracle-
alone check asserts there (>= 2 in all); the shadow cases assert two after the first.
"""
import ctypes
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import magical_amd
import pyoracle as po
from magical_amd import native, registry
from test_gpu_parity import oracle_env, oracle_obs_split

SEED0 = 9100
WORD_LIMIT = 7000          # words one reset may draw: ten whole-layout retries; reaching it is a failure
STREAM_SEEDS = [0, 1, 12345, 2**32 - 1]

REGION_DYN = "MoveToRegion-TestDynamics-LoRes4E-v0"
CORNER_DYN = "MoveToCorner-TestDynamics-LoRes4E-v0"
CORNER_COL = "MoveToCorner-TestColour-LoRes4E-v0"
CORNER_SHAPE = "MoveToCorner-TestShape-LoRes4E-v0"
CORNER_DEMO = "MoveToCorner-Demo-LoRes4E-v0"
MATCH_ALL, CLUSTER_ALL = "MatchRegions-TestAll-LoRes4E-v0", "ClusterColour-TestAll-LoRes4E-v0"
PICK_DEMO = "PickAndPlace-Demo-LoRes4E-v0"

# variant -> (words per reset, steps of its GPU run, the resets after the first that twist, whether those twists fall
# strictly inside the reset (False: on its first draw), whether the resets after a twist start at odd pos)
VARIANTS = {
    REGION_DYN: (10, 130, (63, 125), True, False),
    CORNER_DYN: (14, 95, (45, 90), True, False),
    CORNER_COL: (5, 255, (125, 250), True, True),
    CORNER_SHAPE: (5, 255, (125, 250), True, True),
    CORNER_DEMO: (4, 160, (157,), False, False),
}
_V, _B, _B0 = "MG_STEP_VARIANT", "MG_STEP_BLK", "MG_STEP_BLK0"


# ---------------------------------------------------------------------------
# the reference: numpy
def np_words(seed, k):
    return np.frombuffer(np.random.RandomState(seed).bytes(4 * k), "<u4")


def np_state(rs):
    s = rs.get_state()
    return s[1].copy(), int(s[2])


def assert_rng_equal(got, ref, what=""):
    """(key uint32 [..., 624], pos [...]) of `got` against `ref`, exactly: pos first, then every key word"""
    gk, gp = np.asarray(got[0]), np.asarray(got[1])
    rk, rp = np.asarray(ref[0]), np.asarray(ref[1])
    assert gk.dtype == np.uint32 and rk.dtype == np.uint32, what
    assert gk.shape == rk.shape and gk.shape[-1] == 624 and gp.shape == rp.shape == gk.shape[:-1], what
    bad = np.argwhere(np.atleast_1d(gp != rp))
    assert bad.size == 0, f"{what}: pos {np.atleast_1d(gp)[tuple(bad[0])]} != {np.atleast_1d(rp)[tuple(bad[0])]} at {bad[0]}"
    bad = np.argwhere(gk != rk)
    assert bad.size == 0, f"{what}: key word {bad[0]} (of {len(bad)} that differ)"


def advance_to(rs, key, pos):
    """advance numpy's stream word by word until its state is (key, pos); returns the words drawn"""
    n = 0
    while True:
        k, p = np_state(rs)
        if p == pos and np.array_equal(k, key):
            return n
        assert n < WORD_LIMIT, f"no agreement with numpy's stream within {WORD_LIMIT} words"
        rs.bytes(4)
        n += 1


@functools.lru_cache(maxsize=None)
def fixed_stream(seed, words, resets):
    """numpy's state after 0 .. `resets` resets of `words` words each: (keys [resets + 1, 624], pos [resets + 1])"""
    rs = np.random.RandomState(seed)
    keys, pos = np.empty((resets + 1, 624), dtype=np.uint32), np.empty(resets + 1, dtype=np.int32)
    for k in range(resets + 1):
        if k:
            rs.bytes(4 * words)
        keys[k], pos[k] = np_state(rs)
    keys.setflags(write=False)
    pos.setflags(write=False)
    return keys, pos


class FixedRef:
    """the reference of a variant whose resets all draw `words` words: numpy alone"""

    def __init__(self, seeds, words, resets):
        self.streams = [fixed_stream(int(s), words, resets) for s in seeds]

    def at(self, counts, envs=None):
        envs = range(len(self.streams)) if envs is None else envs
        return (np.stack([self.streams[i][0][counts[i]] for i in envs]),
                np.array([self.streams[i][1][counts[i]] for i in envs], dtype=np.int32))


def twists(pos):
    """the resets (1-based) in which the stream twisted, from pos after 0, 1, .. resets (each reset draws at least one
    word and fewer than 624): those that start at 624 or end at a lower pos than they started"""
    return [k for k in range(1, len(pos)) if pos[k - 1] == 624 or pos[k] < pos[k - 1]]


@functools.lru_cache(maxsize=None)
def oracle_run(name, seeds, resets, watch):
    """`resets` reset() calls of one oracle env per seed: .keys [n, resets + 1, 624], .pos [n, resets + 1] (index 0:
    as seeded), .obs[i][k] the observation (with_targets, deflated) of watched env i after reset k"""
    spec = registry.lookup(name)
    n = len(seeds)
    keys, pos = np.empty((n, resets + 1, 624), dtype=np.uint32), np.empty((n, resets + 1), dtype=np.int32)
    obs = {i: [None] for i in watch}
    for i, seed in enumerate(seeds):
        o = oracle_env(spec, seed)
        keys[i, 0], pos[i, 0] = o.rng_state()
        for k in range(1, resets + 1):
            flat = o.reset()          # PlacementError here: a seed that must not be used
            keys[i, k], pos[i, k] = o.rng_state()
            if i in obs:
                tgt = o.target() if spec.task == "PickAndPlace" else np.zeros(4)
                obs[i].append((zlib.compress(flat.tobytes(), 1), tgt))
    keys.setflags(write=False)
    pos.setflags(write=False)
    return SimpleNamespace(keys=keys, pos=pos, obs=obs, spec=spec)


def run_obs(run, i, k):
    """watched env i's observation dict after its reset k"""
    blob, tgt = run.obs[i][k]
    ref = oracle_obs_split(run.spec, np.frombuffer(zlib.decompress(blob), dtype=np.uint8))
    if run.spec.task == "PickAndPlace":
        t = tgt.astype(np.float32)
        ref["target_type"], ref["target_colour"], ref["target_position"] = t[0:1], t[1:2], t[2:4]
    return ref


def run_at(run, counts):
    n = len(counts)
    return run.keys[np.arange(n), counts], run.pos[np.arange(n), counts]


# ---------------------------------------------------------------------------
# CPU: the oracle against numpy
@pytest.mark.parametrize("seed", STREAM_SEEDS)
def test_oracle_words_match_numpy_over_three_twists(seed):
    mt = po.MT(seed)
    got = np.array([mt.next32() for _ in range(2000)], dtype=np.uint32)
    assert np.array_equal(got, np_words(seed, 2000))


@pytest.mark.parametrize("skip", [623, 1247])
@pytest.mark.parametrize("seed", STREAM_SEEDS)
def test_oracle_draws_straddle_a_twist(seed, skip):
    """double / uniform / randint started on the last word before a twist (a double's two words straddle it; a
    rejected randint word is followed by one from the new block), then 20 more of the same"""
    draws = [("double", lambda m: m.double(), lambda r: r.random_sample()),
             ("uniform", lambda m: m.uniform(-0.73, 2.9), lambda r: r.uniform(-0.73, 2.9))]
    for lo, hi in ((0, 4), (1, 6), (7, 11), (0, 18)):
        draws.append((f"randint({lo},{hi})", lambda m, lo=lo, hi=hi: m.randint(lo, hi),
                      lambda r, lo=lo, hi=hi: int(r.randint(lo, hi))))
    for what, ours, theirs in draws:
        mt, rs = po.MT(seed), np.random.RandomState(seed)
        for _ in range(skip):
            mt.next32()
        rs.bytes(4 * skip)
        assert np_state(rs)[1] == 623
        for k in range(21):
            assert ours(mt) == theirs(rs), (what, k)
        assert np_state(rs)[1] < 623                      # the twist is behind both
        assert mt.next32() == np.frombuffer(rs.bytes(4), "<u4")[0], what     # and they stand at the same word


@pytest.mark.parametrize("name", list(VARIANTS))
def test_oracle_env_resets_follow_numpy(name):
    """after each reset the oracle env's rng_state() is numpy's stream of the same seed some words further on; and what
    the GPU cases of this variant rely on: the words per reset, the resets that twist, where in the reset"""
    words, steps, claimed, inside, odd = VARIANTS[name]
    spec = registry.lookup(name)
    for seed in (SEED0, SEED0 + 16):
        o, rs = oracle_env(spec, seed), np.random.RandomState(seed)
        assert_rng_equal(o.rng_state(), np_state(rs), "seeded")
        pos = [624]
        for k in range(1, steps + 2):
            o.reset()
            key, p = o.rng_state()
            assert advance_to(rs, key, p) == words, (name, seed, k)
            pos.append(p)
        tw = twists(pos)
        assert tw[0] == 1 and tuple(tw[1:]) == claimed, (name, seed, tw)
        assert len(claimed) >= 2 or name == CORNER_DEMO      # (the Demo row's 160 steps hold reset 157 alone)
        for k in claimed:
            assert (pos[k - 1] != 624 and pos[k - 1] + words > 624) == inside, (name, k, pos[k - 1])
            assert inside or pos[k - 1] == 624
        if odd:     # a 5-word reset is two doubles and a randint; after the first twist the resets start at odd and
            # even pos in turn, and the second twisting one starts at an odd pos: the twist splits a double
            assert [p % 2 for p in pos[claimed[0]:claimed[0] + 4]] == [1, 0, 1, 0], name
            assert pos[claimed[1] - 1] in (621, 623), name
        # the fixed-words reference of the GPU cases is this very stream
        keys, fpos = fixed_stream(seed, words, steps + 1)
        assert list(fpos) == pos and np.array_equal(keys[-1], o.rng_state()[0])


def test_state_comparison_bites():
    """assert_rng_equal passes on equal states and fails when the reference is one word ahead, when pos alone
    differs, and when key word 623 alone differs"""
    rs = np.random.RandomState(12345)
    rs.bytes(4 * 1247)                      # pos 623: the next word twists
    key, pos = np_state(rs)
    ahead = np.random.RandomState(12345)
    ahead.bytes(4 * 1248)
    k623 = key.copy()
    k623[623] ^= 1
    cases = {"equal": ((key.copy(), pos), True), "one word ahead": (np_state(ahead), False),
             "pos": ((key.copy(), pos + 1), False), "key word 623": ((k623, pos), False)}
    rs2 = np.random.RandomState(12345)
    rs2.bytes(4 * 700)
    ahead2 = np.random.RandomState(12345)
    ahead2.bytes(4 * 701)                   # one word ahead inside a block: the keys agree, pos does not
    cases["one word ahead, same block"] = (np_state(ahead2), None)
    for what, (ref, ok) in cases.items():
        got = (key, pos) if ok is not None else np_state(rs2)
        try:
            assert_rng_equal(got, ref, what)
            passed = True
        except AssertionError:
            passed = False
        assert passed == bool(ok), what
    # batched, as the GPU tests call it: one env of three off by key word 623
    gk, gp = np.stack([key] * 3), np.array([pos] * 3, dtype=np.int32)
    rk = gk.copy()
    rk[2, 623] ^= 0x80000000
    assert_rng_equal((gk, gp), (gk.copy(), gp.copy()))
    with pytest.raises(AssertionError):
        assert_rng_equal((gk, gp), (rk, gp))


def test_mask_rotation_of_the_explicit_reset_case():
    """every env of the PickAndPlace case is reset 18 to 20 times by the 45 masked calls, none in every call"""
    counts = sum(pick_mask(c, 8).astype(int) for c in range(45))
    assert counts.min() == 18 and counts.max() == 20
    assert all(0 < pick_mask(c, 8).sum() < 8 for c in range(45))


# ---------------------------------------------------------------------------
# GPU
def gpu_rng(vec):
    key, pos = vec.rng_state()
    assert key.dtype == torch.uint32 and pos.dtype == torch.int32
    assert tuple(key.shape) == (vec.num_envs, 624) and tuple(pos.shape) == (vec.num_envs,)
    return key.cpu().numpy(), pos.cpu().numpy()


def assert_obs(obs, i, ref, what):
    for k, v in obs.items():
        assert np.array_equal(v[i].cpu().numpy(), ref[k]), f"{what}: env {i} obs {k}"


def selftest_mt(seeds, ndraws, mode, n=None, null=None, room=None):
    """(return code, the words u32[copies, n, ndraws]) of mg_selftest_mt; `room`: words to allocate for the output"""
    lib = native.load()
    n = len(seeds) if n is None else n
    copies = 2 if mode == 2 else 1
    sd = torch.from_numpy(np.array(seeds, dtype=np.uint32)).cuda()
    out = torch.zeros(room if room is not None else copies * n * ndraws, dtype=torch.uint32, device="cuda")
    rc = lib.mg_selftest_mt(None if null == "seeds" else ctypes.c_void_p(sd.data_ptr()), n, ndraws, mode,
                            None if null == "out" else ctypes.c_void_p(out.data_ptr()),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


SELFTEST_SEEDS = [0, 2**32 - 1, 1, 12345, SEED0, SEED0 + 16, 0x80000000, 19650218]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["hbm-serial", "lds-64-lanes", "lds-37-lanes"])
def test_selftest_mt_words_match_numpy(mode):
    ndraws = 1900           # three twists: before words 0, 624 and 1248
    rc, out = selftest_mt(SELFTEST_SEEDS, ndraws, mode)
    assert rc == 0, native.load().mg_last_error()
    out = out.reshape(-1, len(SELFTEST_SEEDS), ndraws)
    assert out.shape[0] == (2 if mode == 2 else 1)
    for c in range(out.shape[0]):
        for i, seed in enumerate(SELFTEST_SEEDS):
            bad = np.flatnonzero(out[c, i] != np_words(seed, ndraws))
            assert bad.size == 0, f"mode {mode} copy {c} seed {seed}: first wrong word {bad[0]} of {bad.size}"
    if mode == 2:
        assert np.array_equal(out[0], out[1])


@pytest.mark.gpu
def test_selftest_mt_refusals():
    """-22 and nothing launched; the buffers would hold what a call that was not refused writes"""
    room = 2 * 4097 * 8
    seeds = [7] * 4097
    for what, kw in {"n = 0": dict(n=0, ndraws=8, mode=0), "n < 0": dict(n=-1, ndraws=8, mode=1),
                     "n = 4097": dict(n=4097, ndraws=8, mode=1), "ndraws = 0": dict(n=2, ndraws=0, mode=0),
                     "ndraws < 0": dict(n=2, ndraws=-5, mode=2), "ndraws = 8193": dict(n=2, ndraws=8193, mode=2),
                     "mode 3": dict(n=2, ndraws=8, mode=3), "mode -1": dict(n=2, ndraws=8, mode=-1),
                     "null seeds": dict(n=2, ndraws=8, mode=0, null="seeds"),
                     "null out": dict(n=2, ndraws=8, mode=1, null="out")}.items():
        rc, out = selftest_mt(seeds, room=room, **kw)
        assert rc == -22, what
        assert b"mg_selftest_mt" in native.load().mg_last_error(), what
        assert not out.any(), what
    rc, out = selftest_mt(seeds[:4096], 1, 1, room=room)       # the largest n is taken
    assert rc == 0 and np.array_equal(out[:4096], np.full(4096, np_words(7, 1)[0]))


def drive_fixed(monkeypatch, name, n, steps, env=(), form=None, max_episode_steps=1, phases=None, seq=False):
    """A sim of `name` whose resets all draw the variant's words: reset, `steps` steps (seq: step_seq calls of R = 2),
    after each the rng_state() of every env against numpy and the watched envs' observations against the oracle."""
    for k, v in dict(env).items():
        monkeypatch.setenv(k, v)
    words = VARIANTS[name][0]
    spec = registry.lookup(name)
    seeds = [SEED0 + i for i in range(n)]
    vec = magical_amd.make_vec(name, n, seeds=seeds, max_episode_steps=max_episode_steps)
    try:
        if form is not None:
            assert vec.step_form()[:2] == form
        ref = FixedRef(seeds, words, steps + 1)
        watch = sorted({0, n // 2, n - 1})
        orc = {i: oracle_env(spec, seeds[i]) for i in watch}
        acts = np.random.RandomState(7).randint(0, 18, (steps, 2, n) if seq else (steps, n))
        counts = np.zeros(n, dtype=np.int64)
        assert_rng_equal(gpu_rng(vec), ref.at(counts), "seeded")
        obs = vec.reset()
        counts += 1
        assert_rng_equal(gpu_rng(vec), ref.at(counts), "reset")
        for i in watch:
            assert_obs(obs, i, oracle_obs_split(spec, orc[i].reset()), "reset")
        ep = np.zeros(n, dtype=np.int64)
        if phases is not None:
            vec.set_episode_steps(phases)
            ep = np.array(phases, dtype=np.int64)
        for t in range(steps):
            a = torch.as_tensor(acts[t], dtype=torch.uint8)
            if seq:
                obs, rew, done, info = vec.step_seq(a)
                assert bool((info["steps"] == 1).all()), f"call {t}"
            else:
                obs, rew, done, info = vec.step(a)
            ep += 1
            d = ep >= max_episode_steps
            ep[d] = 0
            counts[d] += 1
            assert np.array_equal(done.cpu().numpy().astype(bool), d), f"step {t} done"
            assert_rng_equal(gpu_rng(vec), ref.at(counts), f"step {t}")
            for i in watch:
                if d[i]:
                    want = oracle_obs_split(spec, orc[i].reset())
                    rk, rp = ref.at(counts, [i])
                    assert_rng_equal(orc[i].rng_state(), (rk[0], rp[0]), f"step {t} oracle env {i}")
                    assert_obs(obs, i, want, f"step {t}")
        assert int(vec.errors().abs().sum().item()) == 0
        return counts
    finally:
        vec.close()


FUSED = [(REGION_DYN, (5, 8), 9), (REGION_DYN, (5, 16), 17), (CORNER_DYN, (6, 8), 9), (CORNER_DYN, (6, 16), 17),
         (CORNER_COL, (6, 8), 9), (CORNER_DEMO, (6, 8), 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,n", FUSED, ids=[f"{c[0].split('-')[0]}{c[0].split('-')[1]}-{c[1][0]}/{c[1][1]}-n{c[2]}"
                                                    for c in FUSED])
def test_fused_reset_in_the_step_kernel(monkeypatch, name, form, n):
    """the serial twist over HBM on the env's own lane; the env counts leave the last workgroup ragged, whose shadow
    lanes must not advance env n - 1's stream"""
    counts = drive_fixed(monkeypatch, name, n, VARIANTS[name][1], {_V: str(form[0]), _B: str(form[1])}, form)
    assert (counts == VARIANTS[name][1] + 1).all()


@pytest.mark.gpu
def test_fused_reset_of_desynchronised_envs(monkeypatch):
    """episodes of 2 steps at phases i % 2: in every step, the twisting ones included, every other env of a
    workgroup resets while its neighbours do not"""
    n, steps = 17, 190
    counts = drive_fixed(monkeypatch, CORNER_DYN, n, steps, {_V: "6", _B: "16"}, (6, 16), max_episode_steps=2,
                         phases=[i % 2 for i in range(n)])
    assert counts.min() >= 95 and counts.max() == 96       # past the twists in resets 45 and 90


@pytest.mark.gpu
@pytest.mark.parametrize("env,form", [({"MG_FUSED_RESET": "0", _V: "6", _B: "8"}, (6, 8)), ({_V: "0"}, None)],
                         ids=["fused-reset-off", "hbm-step-form"])
def test_own_launch_auto_reset(monkeypatch, env, form):
    """the same run with the auto-reset as reset_kernel's launch: the cooperative LDS twist"""
    drive_fixed(monkeypatch, CORNER_DYN, 9, VARIANTS[CORNER_DYN][1], env, form)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [CORNER_DYN, REGION_DYN])
def test_step_seq_fused_reset(monkeypatch, name):
    """mg_step_seq, calls of R = 2 on episodes of one step: each call is one env-step and one fused reset"""
    drive_fixed(monkeypatch, name, 9, VARIANTS[name][1], seq=True)


def test_oracle_alone_crosses_twists_in_the_shadow_cases():
    """what the shadow and explicit-reset GPU cases must have compared, from the oracle alone"""
    for name in (MATCH_ALL, CLUSTER_ALL):
        run = oracle_run(name, tuple(SEED0 + i for i in range(9)), 21, (0, 4, 8))
        for i in range(9):
            assert len(twists(list(run.pos[i]))) >= 3, (name, i)      # the first reset's and two more
    run = oracle_run(PICK_DEMO, tuple(SEED0 + i for i in range(8)), 21, (0, 4, 7))
    counts = 1 + sum(pick_mask(c, 8).astype(int) for c in range(45))
    for i in range(8):
        assert len(twists(list(run.pos[i, :counts[i] + 1]))) >= 2, i


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"MG_RESET_PREFETCH": "0"}, {"MG_COPY_WG": "3"}],
                         ids=["shadow", "prefetch-off", "copy-wg-3"])
@pytest.mark.parametrize("name", [MATCH_ALL, CLUSTER_ALL])
def test_next_layout_shadow(monkeypatch, name, env):
    """auto-resets handed over from the next-layout shadow (or run in place): the words per reset vary, so the stream's
    reference is the oracle env's rng_state(), tied to numpy by the CPU tests"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, steps = 9, 20
    seeds = tuple(SEED0 + i for i in range(n))
    watch = (0, n // 2, n - 1)
    run = oracle_run(name, seeds, steps + 1, watch)
    vec = magical_amd.make_vec(name, n, seeds=list(seeds), max_episode_steps=1)
    try:
        acts = np.random.RandomState(7).randint(0, 18, (steps, n))
        counts = np.zeros(n, dtype=np.int64)
        assert_rng_equal(gpu_rng(vec), run_at(run, counts), "seeded")
        obs = vec.reset()
        for t in range(steps + 1):
            if t:
                obs, rew, done, info = vec.step(torch.as_tensor(acts[t - 1], dtype=torch.uint8))
                assert bool(done.all())
            counts += 1
            assert_rng_equal(gpu_rng(vec), run_at(run, counts), f"reset {t + 1}")
            for i in watch:
                assert_obs(obs, i, run_obs(run, i, t + 1), f"reset {t + 1}")
        assert int(vec.errors().abs().sum().item()) == 0
    finally:
        vec.close()


def pick_mask(c, n):
    """the envs call c of the explicit-reset case resets (module docstring)"""
    e = np.arange(n)
    return (e + c // 2) % 2 == 1 if c % 2 == 0 else (e + c // 2) % 3 == 0


@pytest.mark.gpu
def test_explicit_masked_resets():
    """45 reset(mask) calls with rotating masks leave the envs at different pos; each follows its own stream"""
    n, calls = 8, 45
    seeds = tuple(SEED0 + i for i in range(n))
    watch = (0, n // 2, n - 1)
    run = oracle_run(PICK_DEMO, seeds, 21, watch)
    vec = magical_amd.make_vec(PICK_DEMO, n, seeds=list(seeds))
    try:
        obs = vec.reset()
        counts = np.ones(n, dtype=np.int64)
        assert_rng_equal(gpu_rng(vec), run_at(run, counts), "reset")
        for c in range(calls):
            mask = pick_mask(c, n)
            obs = vec.reset(torch.as_tensor(mask))
            counts[mask] += 1
            assert_rng_equal(gpu_rng(vec), run_at(run, counts), f"call {c}")
            for i in watch:
                assert_obs(obs, i, run_obs(run, i, counts[i]), f"call {c}")
        assert len(set(gpu_rng(vec)[1].tolist())) > 1
        assert int(vec.errors().abs().sum().item()) == 0
    finally:
        vec.close()


@pytest.mark.gpu
def test_seeding_robot_scene():
    """seed(): pos 624 and numpy's seeded key before any reset; the following resets draw from the new stream"""
    seeds = [0, 1, 2**32 - 1, 12345, SEED0, SEED0 + 16]
    n, words = len(seeds), VARIANTS[CORNER_DYN][0]
    vec = magical_amd.make_vec(CORNER_DYN, n, seeds=[5] * n, max_episode_steps=1)
    try:
        vec.reset()
        vec.seed(seeds)
        key, pos = gpu_rng(vec)
        assert (pos == 624).all()
        for i, s in enumerate(seeds):
            assert np.array_equal(key[i], np.random.RandomState(s).get_state()[1]), s
        ref = FixedRef(seeds, words, 3)
        assert_rng_equal((key, pos), ref.at([0] * n), "seeded")
        vec.reset()
        assert_rng_equal(gpu_rng(vec), ref.at([1] * n), "reset")
        for t in range(2):
            vec.step(torch.zeros(n, dtype=torch.uint8))
            assert_rng_equal(gpu_rng(vec), ref.at([2 + t] * n), f"step {t}")
    finally:
        vec.close()


@pytest.mark.gpu
def test_reseeding_while_the_shadow_is_live():
    seeds = (0, 1, 2**32 - 1, 12345)
    n, watch = len(seeds), (0, 2, 3)
    run = oracle_run(MATCH_ALL, seeds, 5, watch)
    vec = magical_amd.make_vec(MATCH_ALL, n, seeds=[SEED0 + i for i in range(n)], max_episode_steps=1)
    try:
        vec.reset()
        for t in range(2):      # the shadow holds layouts drawn from the old seeds
            vec.step(torch.zeros(n, dtype=torch.uint8))
        vec.seed(list(seeds))
        key, pos = gpu_rng(vec)
        assert (pos == 624).all()
        for i, s in enumerate(seeds):
            assert np.array_equal(key[i], np.random.RandomState(s).get_state()[1]), s
        assert_rng_equal((key, pos), run_at(run, np.zeros(n, dtype=np.int64)), "seeded")
        # auto-resets in place until the next full reset, then from the re-primed shadow: one stream throughout
        k = 0
        for what in ("step", "step", "reset", "step", "step"):
            obs = vec.reset() if what == "reset" else vec.step(torch.zeros(n, dtype=torch.uint8))[0]
            k += 1
            assert_rng_equal(gpu_rng(vec), run_at(run, np.full(n, k)), f"{what} {k}")
            for i in watch:
                assert_obs(obs, i, run_obs(run, i, k), f"{what} {k}")
    finally:
        vec.close()


@pytest.mark.gpu
def test_snapshot_across_a_twist():
    """a snapshot taken after reset 44 (pos 616), restored into a fresh sim: both draw reset 45 across the twist"""
    n, words = 9, VARIANTS[CORNER_DYN][0]
    seeds = [SEED0 + i for i in range(n)]
    spec = registry.lookup(CORNER_DYN)
    a = magical_amd.make_vec(CORNER_DYN, n, seeds=seeds, max_episode_steps=1)
    b = magical_amd.make_vec(CORNER_DYN, n, seeds=[5] * n, max_episode_steps=1)
    try:
        acts = np.random.RandomState(7).randint(0, 18, (46, n))
        ref = FixedRef(seeds, words, 47)
        watch = (0, n // 2, n - 1)
        orc = {i: oracle_env(spec, seeds[i]) for i in watch}
        a.reset()
        b.reset()
        b.step(torch.as_tensor(acts[0], dtype=torch.uint8))
        for t in range(43):
            a.step(torch.as_tensor(acts[t], dtype=torch.uint8))
        for i in watch:
            for _ in range(44):
                orc[i].reset()
        state = gpu_rng(a)
        assert_rng_equal(state, ref.at([44] * n), "reset 44")
        assert (state[1] == 616).all()
        snap = a.snapshot()
        b.restore(snap)
        assert_rng_equal(gpu_rng(b), state, "restored")
        for t in range(43, 46):
            oa = a.step(torch.as_tensor(acts[t], dtype=torch.uint8))[0]
            ob = b.step(torch.as_tensor(acts[t], dtype=torch.uint8))[0]
            assert_rng_equal(gpu_rng(a), ref.at([t + 2] * n), f"reset {t + 2}")
            assert_rng_equal(gpu_rng(b), ref.at([t + 2] * n), f"reset {t + 2}, restored sim")
            for k in oa:
                assert torch.equal(oa[k], ob[k]), (t, k)
            for i in watch:
                assert_obs(ob, i, oracle_obs_split(spec, orc[i].reset()), f"reset {t + 2}")
    finally:
        a.close()
        b.close()
