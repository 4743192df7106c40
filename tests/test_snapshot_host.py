"""CPU: the host side of env snapshots -- blob sizing (mg_snapshot_bytes touches no GPU), header parsing, save / load."""
import ctypes

import pytest
import torch

from magical_amd import native, registry, snapshot, tables
from magical_amd.snapshot import PoolSnapshot, Snapshot

GPU_PP = {None: 0, "LoRes4E": 1, "LoResStack": 2, "LoRes3EA": 3, "LoRes4A": 4, "LoResCHW4E": 1, "LoResCHW4A": 1}


def snapshot_bytes(name, n):
    spec = registry.lookup(name)
    cfg = native.mg_config(task=spec.task_id, rand_flags=spec.rand_flags, preproc=GPU_PP[spec.preproc], num_envs=64,
                           device=0, max_episode_steps=spec.max_episode_steps, base_seed=0, auto_reset=1, seeds=None,
                           library=None, library_size=ctypes.sizeof(tables.mg_library))
    return native.load().mg_snapshot_bytes(ctypes.byref(cfg), n)


def test_every_test_name_is_registered():
    for name in ("MoveToRegion-Demo-LoRes4E-v0", "MoveToCorner-Demo-LoResStack-v0", "MatchRegions-TestAll-LoResStack-v0",
                 "PickAndPlace-Demo-LoRes4E-v0", "MoveToRegion-Demo-v0", "MoveToCorner-Demo-LoRes3EA-v0",
                 "MoveToRegion-Demo-LoRes4A-v0", "MoveToRegion-Demo-LoResCHW4E-v0", "MatchRegions-TestAll-LoRes4E-v0"):
        assert registry.lookup(name).gpu_supported, name


@pytest.mark.parametrize("name", ["MoveToRegion-Demo-LoRes4E-v0", "ClusterColour-Demo-LoResStack-v0",
                                  "MoveToCorner-Demo-LoRes3EA-v0", "MoveToRegion-Demo-LoRes4A-v0", "MoveToRegion-Demo-v0"])
def test_snapshot_bytes_is_linear_above_the_header(name):
    b = [snapshot_bytes(name, n) for n in (0, 1, 2, 70, 4096)]
    assert b[0] == snapshot.HEADER_BYTES
    rec = b[1] - b[0]
    assert rec > 0 and rec % 16 == 0
    assert b[2] == b[0] + 2 * rec and b[3] == b[0] + 70 * rec and b[4] == b[0] + 4096 * rec
    # at least the frames the preprocessor's stacks need, plus a state section: MT19937 alone is 2500 bytes
    pp = GPU_PP[registry.lookup(name).preproc]
    assert rec >= snapshot.frame_bytes(pp) + 2500
    assert snapshot_bytes(name, -1) < 0


# mg_snapshot_bytes(name, 1) and (name, 70) of the library that wrote blob layout version 1: the row count and the state
# section's bytes are part of the format, wherever layout() lives
PINNED = {"MoveToRegion-Demo-LoRes4E-v0": (190304, 13303616), "ClusterColour-Demo-LoResStack-v0": (245600, 17174336),
          "MoveToCorner-Demo-LoRes3EA-v0": (190304, 13303616), "MoveToRegion-Demo-LoRes4A-v0": (162656, 11368256),
          "MoveToRegion-Demo-v0": (24416, 1691456)}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_snapshot_bytes_is_pinned(name):
    assert (snapshot_bytes(name, 1), snapshot_bytes(name, 70)) == PINNED[name]


def test_record_size_depends_on_the_preprocessor_only():
    """Records are sized per preprocessor (the frames they carry), not per task: the state rows are laid out with the
    same MG_MAX_* caps for a robot scene and a many-block scene."""
    assert snapshot_bytes("MoveToRegion-Demo-LoResStack-v0", 10) == snapshot_bytes("ClusterColour-Demo-LoResStack-v0", 10)
    assert snapshot_bytes("MoveToRegion-Demo-LoRes4E-v0", 10) < snapshot_bytes("MoveToRegion-Demo-LoResStack-v0", 10)
    d = snapshot_bytes("MoveToRegion-Demo-LoResStack-v0", 10) - snapshot_bytes("MoveToRegion-Demo-LoRes4E-v0", 10)
    assert d == 10 * (snapshot.frame_bytes(2) - snapshot.frame_bytes(1))


def _blob(count=3, record_bytes=64, **over):
    fields = dict(task=4, rand_flags=62, preproc=2, max_bodies=16, max_shapes=64, max_cons=32, max_arb=48, max_ents=14,
                  nrows=100, nframes=0, state_bytes=record_bytes, record_bytes=record_bytes, count=count,
                  total_bytes=snapshot.HEADER_BYTES + count * record_bytes)
    fields.update(over)
    body = bytes(range(256)) * ((count * record_bytes + 255) // 256)
    raw = snapshot.pack_header(**fields) + body[:count * record_bytes]
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8)


def test_header_round_trip_and_save_load(tmp_path):
    snap = Snapshot(_blob())
    h = snap.header
    assert (h.magic, h.version, h.task, h.rand_flags, h.preproc) == (snapshot.MAGIC, snapshot.VERSION, 4, 62, 2)
    assert (h.max_bodies, h.max_shapes, h.max_cons, h.max_arb, h.max_ents) == (16, 64, 32, 48, 14)
    assert len(snap) == h.count == 3 and h.total_bytes == snap.blob.numel()
    path = str(tmp_path / "s.pt")
    snap.save(path)
    back = Snapshot.load(path)
    assert torch.equal(back.blob, snap.blob) and back.header == h and len(back) == 3
    assert torch.equal(back.cpu().blob, snap.blob) and torch.equal(back.to("cpu").blob, snap.blob)
    assert Snapshot.frombytes(snap.tobytes()).header == h
    # the file holds a tensor and nothing executable
    assert isinstance(torch.load(path, weights_only=True), torch.Tensor)
    pool = PoolSnapshot([Snapshot(_blob(2)), Snapshot(_blob(1))], [0, 2, 3])
    pool.save(path)
    back = PoolSnapshot.load(path)
    assert back.bounds == [0, 2, 3] and len(back) == 3 and [len(c) for c in back.chunks] == [2, 1]


@pytest.mark.parametrize("what,over", [("magic", dict(magic=0x12345678)), ("version", dict(version=snapshot.VERSION + 1)),
                                       ("count", dict(count=0)), ("size", dict(total_bytes=999))])
def test_bad_header_is_rejected_on_the_host(what, over, tmp_path):
    with pytest.raises(native.NativeError):
        Snapshot(_blob(**over)).header
    path = str(tmp_path / "bad.pt")
    torch.save(_blob(**over), path)
    with pytest.raises(native.NativeError):
        Snapshot.load(path)


def test_truncated_blob_is_rejected_on_the_host():
    blob = _blob()
    with pytest.raises(native.NativeError):
        Snapshot(blob[:-1].clone()).header
    with pytest.raises(native.NativeError):
        Snapshot(blob[:100].clone()).header
