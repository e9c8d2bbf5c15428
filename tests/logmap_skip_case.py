"""Child process of tests/test_gpu_logmap_centers.py: the log-map centres of the sets `skip_sets()` names, one line of digests per
set - run with and without MIDAS_MOMENTS_SKIP=0 (the switch is read once per process), the lines must be equal."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def digests():
    import torch

    from midastouch_amd import ops
    from test_gpu_logmap_centers import build_set, skip_sets
    dev = torch.device("cuda", 0)
    out = []
    for name in skip_sets():
        s = build_set(name)
        c, sd, cnt = ops.cluster_centers(torch.as_tensor(s["poses"]).to(dev), torch.as_tensor(s["w"]).to(dev), torch.as_tensor(s["labels"]).to(dev),
                                         torch.as_tensor(s["label_values"]).to(dev), method="logmap")
        h = hashlib.sha256(c.cpu().numpy().tobytes() + sd.cpu().numpy().tobytes() + cnt.cpu().numpy().tobytes()).hexdigest()
        out.append(f"{name} {h}")
    return out


if __name__ == "__main__":
    print("\n".join(digests()))
