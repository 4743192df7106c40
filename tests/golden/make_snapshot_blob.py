"""Write the snapshot blob fixture of tests/test_snapshot.py::test_blob_format_is_stable (needs a GPU):

    python tests/golden/make_snapshot_blob.py [output directory, default tests/golden]

  * snapshot_blob.json -- the env name, the 3 envs' seeds, the 5 + 3 steps' actions and the recorded envs
  * snapshot_blob.bin  -- the blob of envs [2, 0] after the first 5 steps (MoveToRegion-Demo-v0 has no preprocessor, so
                          a record is its state section only)

The committed pair was written by the library as it stood when MG_SNAP_VERSION became 1; regenerate it only together
with a version bump.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "magical-1_amd"))

META = {"name": "MoveToRegion-Demo-v0", "seeds": [1000, 2001, 3007], "before": 5, "after": 3, "envs": [2, 0]}


def main(out):
    import torch
    from magical_amd import envs as mg_envs
    rs = np.random.RandomState(11)
    acts = rs.randint(0, 18, (META["before"] + META["after"], len(META["seeds"])))
    acts[rs.rand(*acts.shape) < 0.5] = 1   # forward: the robot gets somewhere in 5 steps
    meta = dict(META, actions=acts.tolist())
    env = mg_envs.VecMagicalEnv(meta["name"], len(meta["seeds"]), seeds=meta["seeds"])
    env.reset()
    for t in range(meta["before"]):
        env.step(torch.as_tensor(acts[t], dtype=torch.uint8))
    nbytes = env.snapshot_bytes(len(meta["envs"]))   # zeroed: mg_snapshot leaves the state section's tail padding unwritten
    blob = env.snapshot(envs=meta["envs"], out=torch.zeros(nbytes, dtype=torch.uint8, device="cuda")).blob.cpu().numpy()
    env.close()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "snapshot_blob.json"), "w") as f:
        json.dump(meta, f)
        f.write("\n")
    blob.tofile(os.path.join(out, "snapshot_blob.bin"))
    print("snapshot_blob.bin:", blob.size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
