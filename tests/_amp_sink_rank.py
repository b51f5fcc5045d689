"""One rank of tests/test_gpu_amp.py's accumulation test (started as a fresh child process; not collected by pytest).

    python tests/_amp_sink_rank.py <port> <out.npz> <precision>

A single gloo rank on cuda:0 with a GradSync gradient sink: tiny CubeNET(6,1,64) as ONE autograd node, two backwards -- the first
inside ``no_sync()`` -- then ``finish()``.  Saves the buckets' gradients and the two single-step gradients of the plain loop (no
sink) on the same inputs; the parent compares the buckets with the sum of the latter."""
import os
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    port, out, prec = sys.argv[1], sys.argv[2], sys.argv[3]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    dist.init_process_group("gloo", rank=0, world_size=1)
    import hyperpri_amd as H
    from hyperpri_amd.ddp import GradSync
    from oracle import hyperpri_oracle as O        # inputs only: the counter-based generator

    def u(seed, shape):
        return torch.from_numpy(O._u(seed, int(np.prod(shape))).reshape(shape).copy())

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    net = H.CubeNET(6, 1, first_depth=64, bilinear=False)
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in net.state_dict().items())
    net.load_state_dict(O.synth_state_dict(shapes))
    net = H.set_precision(net.to(dev).train(), prec)
    xs = [u(1235 + k, (2, 1, 6, 36, 50)).to(dev) for k in range(2)]
    ms = [(u(4321 + k, (2, 1, 36, 50)) > 0.9).float().to(dev) for k in range(2)]
    crit = torch.nn.BCEWithLogitsLoss()
    res = {}
    for k in range(2):                                   # the plain loop: one step per input, no sink
        for p in net.parameters():
            p.grad = None
        crit(net(xs[k]), ms[k]).backward()
        torch.cuda.synchronize()
        for name, p in net.named_parameters():
            res[f"step{k}/" + name] = p.grad.detach().cpu().numpy()
    for p in net.parameters():
        p.grad = None
    sync = GradSync(net, bucket_mb=4.0, tail_mb=0.25)
    with sync.no_sync():
        crit(net(xs[0]), ms[0]).backward()
        sync.finish()
    crit(net(xs[1]), ms[1]).backward()
    sync.finish()
    torch.cuda.synchronize()
    for name, p in net.named_parameters():
        res["acc/" + name] = p.grad.detach().cpu().numpy()
    res["buckets"] = len(sync.buckets)
    np.savez(out, **res)
    sync.remove()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
