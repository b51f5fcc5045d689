"""Cases shared by test_sort_cpu.py and test_gpu_sort.py: key sets for the device sort (each chosen to break one thing), inputs of
the Lovasz hinge, and the published formulation of that loss in torch (fp64, autograd) that the numpy reference is held against."""
import numpy as np
import torch

KEY_SETS = ("distinct", "equal", "three", "low_byte", "high_byte", "special", "sorted", "reversed")


def lengths(T):
    """One group of each of these lengths (T: the keys one workgroup ranks per pass)."""
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]


def keys(name, n, seed=0):
    """n fp32 keys of key set `name`."""
    rng = np.random.RandomState(seed * 1009 + n % 997)
    if name == "distinct":                                  # a random permutation of distinct values: the basic order
        return (rng.permutation(n).astype(np.float32) - np.float32(n // 2)) * np.float32(0.25)
    if name == "equal":                                     # stability is all that is left
        return np.full(n, 1.5, dtype=np.float32)
    if name == "three":                                     # long tie runs that cross workgroups
        return np.array([-2.0, 0.5, 7.0], dtype=np.float32)[rng.randint(0, 3, n)]
    if name == "low_byte":                                  # one digit carries the order
        return (np.uint32(0x3F800000) + rng.randint(0, 256, n).astype(np.uint32)).view(np.float32)
    if name == "high_byte":                                 # the highest byte only: sign and the upper exponent bits (no inf / NaN)
        return (rng.choice(np.r_[0:127, 128:255], n).astype(np.uint32) << np.uint32(24)).view(np.float32)
    if name == "special":
        sub = np.array([1], dtype=np.uint32).view(np.float32)[0]
        pool = np.array([0.0, -0.0, sub, -sub, np.inf, -np.inf, np.nan, 1.0, -1.0], dtype=np.float32)
        out = pool[rng.randint(0, pool.size, n)].copy()
        bits = out.view(np.uint32)
        nan = np.isnan(out)
        bits[nan] |= rng.randint(0, 2, int(nan.sum())).astype(np.uint32) << np.uint32(31)       # NaNs of both signs
        return out
    if name == "sorted":
        return np.arange(n, dtype=np.float32) * np.float32(0.5) - np.float32(3)
    if name == "reversed":
        return (np.arange(n, dtype=np.float32) * np.float32(0.5) - np.float32(3))[::-1].copy()
    raise KeyError(name)


def torch_order(k, descending):
    """(indices, sorted keys) of torch's stable CPU sort along the last axis."""
    v, i = torch.sort(torch.from_numpy(np.ascontiguousarray(k)), dim=-1, descending=descending, stable=True)
    return i.numpy().astype(np.int32), v.numpy()


# ---- Lovasz hinge ------------------------------------------------------------------------------------------------------------------
def lovasz_torch(x, y, per_image=True, ignore_index=None):
    """The published formulation (Berman et al.: lovasz_hinge / lovasz_hinge_flat / lovasz_grad) in fp64 on the CPU, with the mean
    over the groups of this package (a group with nothing left counts 0): (loss, d loss / d x) as numpy arrays."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).clone().requires_grad_(True)
    yt = torch.from_numpy(np.asarray(y, dtype=np.float64))
    rows = xt.shape[0] if per_image else 1
    total = xt.sum() * 0
    for lg, lb in zip(xt.reshape(rows, -1), yt.reshape(rows, -1)):
        if ignore_index is not None:
            keep = lb != ignore_index
            lg, lb = lg[keep], lb[keep]
        if lg.numel() == 0:
            continue
        lb = (lb >= 0.5).to(torch.float64)
        errors = 1.0 - lg * (2.0 * lb - 1.0)
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        gt_sorted = lb[perm]
        gts = gt_sorted.sum()
        intersection = gts - gt_sorted.cumsum(0)
        union = gts + (1.0 - gt_sorted).cumsum(0)
        jaccard = 1.0 - intersection / union
        if jaccard.numel() > 1:
            jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
        total = total + torch.dot(torch.relu(errors_sorted), jaccard.detach())
    loss = total / rows
    loss.backward()
    return float(loss.detach()), xt.grad.numpy()


def exact_case(shape, seed, positive=0.4):
    """x_i = s_i (1 - k_i / 1024) with k a permutation of distinct integers around 0 inside every group that a sort may see (the
    whole batch): e_i = k_i / 1024 exactly in fp32 and in fp64, no ties."""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    y = (rng.rand(n) < positive).astype(np.float32)
    k = (rng.permutation(n) - n // 2).astype(np.float64)
    s = np.where(y >= 0.5, 1.0, -1.0)
    x = (s * (1.0 - k / 1024.0)).astype(np.float32)
    assert np.array_equal((1.0 - x.astype(np.float64) * s) * 1024.0, k)
    return x.reshape(shape), y.reshape(shape)
