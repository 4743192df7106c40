"""The quad step forms' solver sweep with streamed joint rows (csrc/mg_step.h, static_solve) against the oracle.

Forms 5/8 and 6/8 read each joint row's pre-stepped terms from the LDS view one row ahead of use instead of holding
them in registers for the ten iterations (5/16 and 6/16 keep the held rows); all four are forced here through
MG_STEP_VARIANT / MG_STEP_BLK at 9 and 17 envs (a ragged last workgroup: one real env plus shadows) over 45 steps, so
MoveToRegion crosses its 40-step episode boundary through the fused reset.

Inputs.  Env i is seeded SEEDS[i] = 9300 + k and follows plan k % len(PLANS[scene]): way-points towards which a steering rule
(steer) turns and drives the oracle's robot, the actions it takes being recorded and then played to the GPU (action =
move (0 none, 1 forward, 2 back) + 3 * turn (0 none, 1 left, 2 right) + 9 * fingers closed).
  * MoveToRegion: fingers closed, diagonally into the top left corner -- a wall first (one arbiter), then both (two) --
    straight back out (none), then towards a wall again until the episode ends.
  * MoveToCorner: into the top wall or a top corner, then across the arena against the block and with it into the
    bottom wall (robot-block and block-wall arbiters together); or to the block first and with it into a bottom corner.
After every step bodies, arbiter tables (mg_get_arbiters), reward, done and eval_score are compared with the oracle
(bodies and contact fields within 1e-9, everything else equal: the bounds of test_step_kernel_forms and
assert_twin_step).  The CPU test asserts on the oracle alone that every env meets zero, one and two or more live
arbiters; the GPU test asserts it again on what it compared.

Register budget (CPU test on the built library's kernel notes): step_kernel<5,8> and <6,8> take at most 368 unified
registers (VGPR + AGPR, rounded up to the granule of 8), which leaves room on the SIMD for two 72-register render
wavefronts, and no more scratch than the held-row kernels did (1264 B per lane each; 442 and 508 registers).
"""
import functools
import math
import os
import re
import struct
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest

from magical_amd import registry
from test_gpu_parity import POSE_TOL, oracle_env
from test_oracle_narrowphase import assert_twin_step, gpu_tables, new_seen, oracle_tables

REGION, CORNER = "MoveToRegion-Demo-LoRes4E-v0", "MoveToCorner-Demo-LoRes4E-v0"
STEPS, NMAX, SEED0 = 45, 17, 9300
# env i's seed (9312 left out: its MoveToCorner layout keeps plan 0's robot off a second arbiter)
SEEDS = [SEED0 + k for k in range(NMAX + 1) if k != 12]
_V, _B = "MG_STEP_VARIANT", "MG_STEP_BLK"
CASES = [(name, (form, blk), n) for name, form in ((REGION, 5), (CORNER, 6)) for blk in (8, 16) for n in (9, 17)]
IDS = [f"{name.split('-')[0]}-{pair[0]}/{pair[1]}-n{n}" for name, pair, n in CASES]

# per scene, plans of (x, y, steps, fingers closed): steer towards (x, y) -- None: straight back -- for `steps` steps
PLANS = {
    REGION: [
        [(-0.4, 0.4, 10, 1), (-1.3, 1.3, 18, 1), (None, None, 5, 0), (0.0, 1.3, 12, 0)],
    ],
    CORNER: [
        [(1.3, 1.3, 16, 0), (0.1, -0.65, 40, 0)],
        [(-1.3, 1.3, 17, 0), (0.1, -0.65, 40, 1)],
        [(0.1, -0.65, 22, 0), (0.1, -1.3, 10, 0), (1.3, -1.3, 20, 0)],
    ],
}


def steer(o, r0, target, closed):
    """the action that turns the robot (body r0 of oracle env `o`) towards `target` and drives once it roughly faces it"""
    if target[0] is None:
        return 2 + 9 * closed
    bx, by, a = o.bodies()[r0, :3]
    want = math.atan2(-(target[0] - bx), target[1] - by)     # forward is the body's local +y
    err = (want - a + math.pi) % (2 * math.pi) - math.pi
    turn = 0 if abs(err) < 0.15 else 3 if err > 0 else 6
    return (1 if abs(err) < 0.9 else 0) + turn + 9 * closed


@functools.lru_cache(maxsize=None)
def reference(name):
    """The NMAX oracle envs of a scene steered through their plans (shared by the scene's cases; read only): per env
    (.acts, .steps = per step (oracle_tables, reward, done, score), .rob = the robot's bodies)."""
    spec = registry.lookup(name)
    out = []
    for i in range(NMAX):
        o = oracle_env(spec, SEEDS[i])
        o.reset()
        nb, r0 = 0, None
        for kind in o.entities()[0]:   # bodies in entity add order: blocks 1, robot 6, others 0
            if kind == 2:
                r0 = nb
            nb += 1 if kind == 3 else 6 if kind == 2 else 0
        plan = PLANS[name][(SEEDS[i] - SEED0) % len(PLANS[name])]
        sched = [(x, y, c) for x, y, k, c in plan for _ in range(k)]
        acts, steps = [], []
        for t in range(STEPS):
            x, y, c = sched[min(t, len(sched) - 1)]
            a = steer(o, r0, (x, y), c)
            _, r, d, s = o.step(a)
            if d:
                o.reset()
            acts.append(a)
            steps.append((oracle_tables(o), float(r), bool(d), float(s)))
        out.append(SimpleNamespace(acts=np.array(acts, dtype=np.uint8), steps=steps, rob=set(range(r0, r0 + 6))))
    return out


def live_counts(steps):
    return [len(tab[1]) for tab, _, _, _ in steps]


def assert_exercised(name, live):
    """live[t][i]: arbiters of env i after step t -- every env meets none, one, and two or more"""
    live = np.asarray(live)
    for i in range(live.shape[1]):
        col = live[:, i]
        assert (col == 0).any() and (col == 1).any() and (col >= 2).any(), f"{name} env {i}: live arbiters {list(col)}"
    assert (live >= 2).any()


@pytest.mark.parametrize("name", [REGION, CORNER])
def test_scripts_reach_the_arbiter_rows_on_the_oracle(name):
    ref = reference(name)
    assert_exercised(name, np.array([live_counts(rec.steps) for rec in ref]).T)
    dones = [[d for _, _, d, _ in rec.steps] for rec in ref]
    if name == REGION:      # the 40-step episode boundary, and steps after it
        assert all(row[39] and not any(row[40:]) for row in dones)
    if name == CORNER:      # the block takes part: an arbiter between a robot body and the block, one of the block alone
        for i, rec in enumerate(ref):
            pairs = {(int(w[3]), int(w[4])) for tab, _, _, _ in rec.steps for w in tab[1]}
            assert any((a in rec.rob) != (b in rec.rob) and a >= 0 and b >= 0 for a, b in pairs), f"env {i}: {pairs}"


@pytest.mark.gpu
@pytest.mark.parametrize("name,pair,n", CASES, ids=IDS)
def test_streamed_rows_match_the_oracle(name, pair, n, monkeypatch):
    import torch
    import magical_amd
    monkeypatch.setenv(_V, str(pair[0]))
    monkeypatch.setenv(_B, str(pair[1]))
    ref = reference(name)[:n]
    acts = np.stack([rec.acts for rec in ref], axis=1)
    vec = magical_amd.make_vec(name, n, seeds=SEEDS[:n])
    assert vec.step_form()[:2] == pair
    vec.reset()
    seen = new_seen()
    live = np.zeros((STEPS, n), dtype=int)
    for t in range(STEPS):
        _, rew, done, info = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
        got = gpu_tables(vec)
        rew, done, score = rew.cpu().numpy(), done.cpu().numpy(), info["eval_score"].cpu().numpy()
        want = [rec.steps[t] for rec in ref]
        for i, (_, r, d, s) in enumerate(want):
            assert bool(done[i]) == d, f"step {t} env {i} done"
            assert score[i] == s and rew[i] == np.float32(r), f"step {t} env {i} score {score[i]} vs {s}"
        assert POSE_TOL == 1e-9     # assert_twin_step's bound on bodies is the forms test's
        if any(w[2] for w in want):     # a fresh episode's state is the reset's, not the step's (as the forms test)
            assert all(w[2] for w in want)
        else:
            assert_twin_step(t, got, [w[0] for w in want], [rec.rob for rec in ref], seen)
        live[t] = got[1][:, 3]
    print(name, pair, n, seen)
    assert_exercised(name, live)
    assert seen["arbiters"] > 0 and seen["wall"] > 0 and seen["robot"] > 0
    assert int(vec.errors().abs().sum().item()) == 0
    vec.close()


# ---------------------------------------------------------------------------
# register budget, from the built library's kernel notes
LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "magical-1_amd", "magical_amd",
                   "libmagical_sim.so")
BUDGET = 368            # + two 72-register render wavefronts = 512, a SIMD's unified register file
HELD_SCRATCH = 1264     # bytes per lane of step_kernel<5,8> and <6,8> with the rows held (442 / 508 registers)


def _readelf():
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm"), "/opt/rocm"):
        p = os.path.join(d, "llvm", "bin", "llvm-readelf")
        if os.path.exists(p):
            return p
    return None


def kernel_notes(path, readelf):
    """{kernel symbol: {note field: int}} of the gfx code objects bundled in the library"""
    data = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, pos = {}, 0
    while True:
        at = data.find(magic, pos)
        if at < 0:
            break
        pos = at + len(magic)
        (count,) = struct.unpack_from("<Q", data, at + 24)
        p = at + 32
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen]
            p += 24 + tlen
            if b"amdgcn" not in triple or not size:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(data[at + off:at + off + size])
                f.flush()
                txt = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True, check=True).stdout
            for blk in re.split(r"\n\s+- \.agpr_count:", txt)[1:]:
                blk = ".agpr_count:" + blk.split("amdhsa.target")[0]
                f_ = {k: v for k, v in re.findall(r"\.(\w+):\s+(\S+)", blk)}
                out[f_["name"]] = {k: int(v) for k, v in f_.items() if v.isdigit()}
    return out


def test_step_kernels_leave_room_for_two_render_waves():
    readelf = _readelf()
    if not os.path.exists(LIB) or readelf is None:
        pytest.skip("the library (or llvm-readelf) is absent")
    notes = kernel_notes(LIB, readelf)
    for form in (5, 6):
        k = [v for name, v in notes.items() if name.startswith(f"_Z11step_kernelILi{form}ELi8EE")]
        assert len(k) == 1, f"step_kernel<{form}, 8> not found among {len(notes)} kernels"
        regs = (k[0]["vgpr_count"] + 7) // 8 * 8       # on gfx950 the note's vgpr_count is the unified VGPR + AGPR total
        print(f"step_kernel<{form}, 8>: {k[0]['vgpr_count']} registers ({k[0]['agpr_count']} AGPR), "
              f"scratch {k[0]['private_segment_fixed_size']} B")
        assert k[0]["vgpr_count"] >= k[0]["agpr_count"]
        assert regs <= BUDGET, f"step_kernel<{form}, 8>: {regs} registers"
        assert k[0]["private_segment_fixed_size"] <= HELD_SCRATCH, f"step_kernel<{form}, 8> scratch"
