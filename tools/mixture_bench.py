#!/usr/bin/env python3
"""Spectral Gaussian mixtures (hyperpri_amd/mixture.py): what a score pass and a fitting pass cost on the card, in the manner of
tools/cluster_probe.py (its timing: device events over ``--calls`` back-to-back calls, legs interleaved round by round).

    python tools/mixture_bench.py                  # one MI355X; writes profiles/mixture.json

On slots of 608 x 968 x 238 (channel stride 240, fp32) at (K, q) in {(2, 8), (8, 8), (2, 32), (8, 32)}, each ``[median, min, max]`` ms:

* ``score``: ``hpri_band_gmm_score`` (the logit of a two-class model) on a gathered batch of two cubes; ``project``:
  ``hpri_band_project`` at the same q on that batch (stage 1 alone);
* ``sums``: one ``hpri_band_gmm_sums`` pass over four slots;
* ``moments``: ``hpri_band_moments`` over the same slots -- one memory-bound read of the same bytes;
* ``composite``: the same work from torch operators: ``addmm``, a batched product with A_k, ``logsumexp``, and for the sums
  ``softmax`` and ``einsum`` for the weighted moments; ``differs``: the largest difference between kernel and composite.

Each step runs in a child process under a time limit; the second is not started when the first fails.  Nothing is gated.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cluster_probe as P  # noqa: E402  (the timing helpers and the shapes)

H, W, BANDS, FIT_SLOTS, BATCH = P.H, P.W, P.BANDS, P.FIT_SLOTS, P.BATCH
SETTINGS = ((2, 8), (8, 8), (2, 32), (8, 32))
STEP_SECONDS = 300


def _setup(n):
    """A filled cache and, per setting, a two-class model on a whitened PCA of it: means from seeded sample pixels, covariances
    0.5 I plus a seeded positive semi-definite perturbation."""
    import numpy as np
    import torch
    from hyperpri_amd import cluster as C
    from hyperpri_amd import mixture as M
    from hyperpri_amd import spectral as S
    from hyperpri_amd.cache import CubeCache
    from hyperpri_amd.engine import synth_fill_
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cache = CubeCache(n, H, W, BANDS, device=dev)
    raw = torch.empty((H, W, BANDS), dtype=torch.float32, device=dev)
    m = torch.empty((H, W), dtype=torch.float32, device=dev)
    for k in range(n):
        synth_fill_(raw, 1234 + k, mode=0)
        synth_fill_(m, 4321 + k, mode=1, thr=0.9)
        cache.put(k, raw, m, name=f"cube{k}")
    stats = S.band_statistics(cache)
    pivot = stats.mean.astype(np.float32)
    sample = C._sample_pixels(cache, list(range(n)), 0, 0) - pivot.astype(np.float64)
    models = {}
    for K, q in SETTINGS:
        w = S.pca_basis(stats, q, whiten=True)[0]
        rng = np.random.default_rng(10 * K + q)
        means = (sample @ w.astype(np.float64).T)[rng.choice(len(sample), size=K, replace=False)]
        g = 0.1 * rng.standard_normal((K, q, q))
        models[f"k{K}_q{q}"] = M.SpectralGMM(pivot, w, means, 0.5 * np.eye(q)[None] + g @ g.transpose(0, 2, 1), np.full(K, 1.0 / K),
                                           np.arange(K) % 2).to(dev)
    mom = S._Pass(cache, list(range(n)))
    count = torch.empty(1, dtype=torch.int64, device=dev)
    msum = torch.empty(cache.cs, dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def moments():
        from hyperpri_amd import _lib
        from hyperpri_amd.engine import _p
        _lib.call("hpri_band_moments", *mom.head, 0, None, _p(mom.work), mom.nbytes, _p(count), _p(msum), None, stream)
    return dev, cache, models, moments, stream


def _terms(model, dev, cs):
    """``xf (P, cs) -> (z, l (P, K))`` from torch operators."""
    import torch
    pv, wd, A, a, c, _ = model._device(dev, cs)
    shift = -(wd @ pv)

    def terms(xf):
        z = torch.addmm(shift, xf, wd.t())
        u = torch.einsum("kij,pj->pki", A, z) + a
        return z, c - 0.5 * (u * u).sum(dim=2)
    return terms


def _report(legs, differs, rounds, calls, pixels, cs):
    ms = {k: [v["median"], v["min"], v["max"]] for k, v in P._measure(legs, rounds, calls).items()}
    return {"pixels": pixels, "bytes_read": pixels * cs * 4, "ms": ms, "differs": differs}


def step_score(rounds, calls):
    import torch
    from hyperpri_amd import spectral as S
    dev, cache, models, moments, _ = _setup(BATCH)
    cs, pixels = cache.cs, BATCH * H * W
    x = cache.batch(list(range(BATCH)))["image"]
    xf = torch.as_strided(x, (pixels, cs), (cs, 1))
    legs, differs = {"moments": moments}, {}
    for tag, model in models.items():
        proj = S.SpectralProjection(model.weight, torch.zeros(model.q)).to(dev)
        terms, cls = _terms(model, dev, cs), model.classes.to(dev)

        def composite(terms=terms, cls=cls):
            l = terms(xf)[1]
            return torch.logsumexp(l[:, cls == 1], dim=1) - torch.logsumexp(l[:, cls == 0], dim=1)
        legs[f"score_{tag}"] = lambda model=model: model(x, output="logit")
        legs[f"project_q{model.q}"] = lambda proj=proj: proj(x)
        legs[f"composite_{tag}"] = composite
        differs[tag] = {"logit": float((legs[f"score_{tag}"]().reshape(-1) - composite()).abs().max())}
    return _report(legs, differs, rounds, calls, pixels, cs)


def step_sums(rounds, calls):
    import numpy as np
    import torch
    from hyperpri_amd import _lib
    from hyperpri_amd import mixture as M
    from hyperpri_amd.engine import _p
    dev, cache, models, moments, stream = _setup(FIT_SLOTS)
    cs, pixels, idx = cache.cs, FIT_SLOTS * H * W, list(range(FIT_SLOTS))
    xf = cache._cubes[:FIT_SLOTS].reshape(pixels, cs)
    legs, differs = {"moments": moments}, {}
    for tag, model in models.items():
        K, q = model.k, model.q
        ps = M._GmmPass(cache, idx, q, K)
        ops = M._device_operands(model.operands, dev, cs)
        terms, means = _terms(model, dev, cs), ops[5][:, :q]

        def sums(ps=ps, ops=ops, K=K, q=q):
            pv, w, A, a, c, m = ops
            base, qp = ps.out.data_ptr(), ps.qp
            oQ = base + 8 * (1 + K + K * qp)
            _lib.call("hpri_band_gmm_sums", *ps.head, 0, _p(pv), _p(w), q, _p(A), _p(a), _p(c), _p(m), K, _p(ps.work), ps.nbytes, base, base + 8,
                      base + 8 * (1 + K), oQ, oQ + 8 * K * qp * qp, stream)

        def composite(terms=terms, means=means, q=q):
            z, l = terms(xf)
            r = torch.softmax(l, dim=1)
            e = z[:, None, :q] - means[None]
            re = r[:, :, None] * e
            return r.sum(dim=0), re.sum(dim=0), torch.einsum("pki,pkj->kij", re, e), torch.logsumexp(l, dim=1).sum()
        legs[f"sums_{tag}"], legs[f"composite_{tag}"] = sums, composite
        sums()
        got, want = ps.out.cpu().numpy(), composite()
        differs[tag] = {"N_over_pixels": float(np.abs(got[1:1 + K] - want[0].double().cpu().numpy()).max() / pixels),
                        "LL_relative": float(abs(got[-1] - float(want[3].double())) / abs(got[-1]))}
    return _report(legs, differs, rounds, calls, pixels, cs)


STEPS = {"score": step_score, "sums": step_sums}


def _dump(rep, fh):
    """One line per leg: the file stays readable and short."""
    lines = []
    for k, v in rep.items():
        if isinstance(v, dict):
            inner = ",\n".join(f'  {json.dumps(a)}: {{\n' + ",\n".join(f"   {json.dumps(c)}: {json.dumps(d)}" for c, d in b.items()) + "\n  }"
                               if isinstance(b, dict) else f"  {json.dumps(a)}: {json.dumps(b)}" for a, b in v.items())
            lines.append(f" {json.dumps(k)}: {{\n{inner}\n }}")
        else:
            lines.append(f" {json.dumps(k)}: {json.dumps(v)}")
    fh.write("{\n" + ",\n".join(lines) + "\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixture.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2, help="back-to-back calls per timed run")
    ap.add_argument("--step", choices=sorted(STEPS), help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            sys.exit("mixture_bench: needs an MI355X (no CPU fallback: a CPU timing says nothing about the GPU)")
        rep = STEPS[args.step](args.rounds, args.calls)
        rep["device"] = torch.cuda.get_device_name(0)
        print("MIXTURE_BENCH " + json.dumps(rep))
        return 0
    rep = {"channel_stride": (BANDS + 7) // 8 * 8, "rounds": args.rounds, "calls_per_round": args.calls, "ms_are": "[median, min, max]"}
    for name in ("score", "sums"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--rounds", str(args.rounds), "--calls", str(args.calls)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            sys.exit(f"mixture_bench: step {name} ran into its limit of {STEP_SECONDS} s; nothing more is started")
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("MIXTURE_BENCH ")), None)
        if r.returncode != 0 or line is None:
            sys.exit(f"mixture_bench: step {name} failed (exit {r.returncode}); nothing more is started\n{r.stdout[-3000:]}")
        rep[name] = json.loads(line[len("MIXTURE_BENCH "):])
        rep["device"] = rep[name].pop("device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        _dump(rep, fh)
    print(json.dumps({name: {k: v[0] for k, v in rep[name]["ms"].items()} for name in ("score", "sums")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
