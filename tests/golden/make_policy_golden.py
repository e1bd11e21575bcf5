"""Writes tests/golden/ppo_2975000_policy.npz from the reference's shipped checkpoint (examples/PPO_2975000.zip):
the 13 policy tensors under their stable-baselines3 names, the checkpoint's sixteen last observations, and the policy's
float64 outputs on them computed here with torch (independent of oracle/policy_oracle.py).  DATA ONLY: the archive's
`data` member (third-party docstrings, pickled code objects) is not copied.  Needs the reference checkout; run by hand:

    python tests/golden/make_policy_golden.py <path to PPO_2975000.zip>
"""
import base64
import io
import json
import os
import pickle
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(path):
    with zipfile.ZipFile(path) as z:
        data = json.loads(z.read("data").decode())
        sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
        version = z.read("_stable_baselines3_version").decode().strip()
    # `_last_obs` is a pickled numpy array (numpy alone unpickles it): the one blob this script opens
    last_obs = np.asarray(pickle.loads(base64.b64decode(data["_last_obs"][":serialized:"])), dtype=np.float32)
    assert last_obs.shape == (16, 8), last_obs.shape
    t = {k: v.double() for k, v in sd.items()}
    x = torch.from_numpy(last_obs).double()

    def net(prefix, head):
        h, i = x, 0
        while f"{prefix}.{i}.weight" in t:
            h = torch.tanh(torch.nn.functional.linear(h, t[f"{prefix}.{i}.weight"], t[f"{prefix}.{i}.bias"]))
            i += 2
        return torch.nn.functional.linear(h, t[head + ".weight"], t[head + ".bias"])

    mean64 = net("mlp_extractor.policy_net", "action_net").numpy()
    value64 = net("mlp_extractor.value_net", "value_net").numpy()[:, 0]
    meta = json.dumps(dict(sb3_version=version, num_timesteps=data.get("num_timesteps"), use_sde=data.get("use_sde")))
    out = {k: v.numpy().astype(np.float32) for k, v in sd.items()}
    assert len(out) == 13, sorted(out)
    np.savez_compressed(os.path.join(HERE, "ppo_2975000_policy.npz"), last_obs=last_obs, mean64=mean64, value64=value64,
                        meta=np.array(meta), **out)


if __name__ == "__main__":
    main(sys.argv[1])
