"""Generates tests/golden/calibrate_ref.npz from the reference's OWN SimQuant.quantize
(/root/reference/quant/kvquant/simquant_module_quantizer.py imported here; nothing is copied):
seeded activations -> the quantizer tuple (upper, lower, signposts) of every calibration configuration that
tests/test_calibrate_cpu.py checks kvquant_amd.calibrate against (plain K pass at 2 and 4 bit, capped outliers with
the first tokens of every sample excluded, Fisher-weighted k-means, the per-token V pass).
k-means sums its partial centroids per OpenMP thread and stops after at most 50 iterations, so its signposts move
with the thread count by about its own tolerance: the fixture is made, and compared against, on one thread.
Run in the build container:  python tests/golden/gen_calibrate.py"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn
from threadpoolctl import threadpool_limits

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/quant/kvquant/simquant_module_quantizer.py"
GOLD = os.path.join(HERE, "calibrate_ref.npz")


def data(seed=0, T=2048, C=256):
    """heavy-tailed activations [T, C] with per-channel scales and offsets.  Drawn in float64 by numpy's PCG64 (its own
    scalar code) with correctly rounded arithmetic only, then rounded once to float32: the same bits on every CPU,
    which torch's vectorised randn / exp (chosen by the CPU's instruction set) do not give"""
    rng = np.random.default_rng(seed)
    scale = rng.lognormal(0.0, 0.5, C)
    shift = 0.2 * rng.standard_normal(C)
    x = rng.standard_normal((T, C)) * scale + shift
    x[rng.random((T, C)) < 0.01] *= 5
    return torch.from_numpy(x.astype(np.float32))


def fisher():
    u = np.random.default_rng(8).random((2048, 64))
    u2 = u * u
    return torch.from_numpy((u2 * u2 + 1e-4).astype(np.float32))


# name -> (data kwargs, bits, qchannel, samples the rows are added in, quantize kwargs besides the common ones)
CASES = {
    "simquant_b2": (dict(seed=2), 2, 0, 1, dict()),
    "simquant_b4": (dict(seed=4), 4, 0, 1, dict()),
    # SQ:421-461 + 441-446 / 487-491: the reference hard-codes 16 samples x 2048 tokens = 32768 rows
    "capped": (dict(seed=5, T=32768, C=24), 2, 0, 16, dict(cap_outliers=True, first_few_fp16=5)),
    "fisher": (dict(seed=7, T=2048, C=64), 3, 0, 1, dict(fisher="fisher")),
    "value": (dict(seed=9, T=512, C=256), 4, -1, 1, dict()),
}


def one_thread():
    return threadpool_limits(limits=1)


def load_ref():
    spec = importlib.util.spec_from_file_location("ref_sq", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run_ref(ref, name):
    dkw, bits, qchannel, nsamples, qkw = CASES[name]
    x = data(**dkw)
    sq = ref.SimQuant(nn.Linear(8, x.shape[1], bias=False), bits, perchannel=True, qchannel=qchannel)
    if nsamples == 1:
        sq.add_batch(None, x.clone())
    else:
        n = x.shape[0] // nsamples
        for i in range(nsamples):
            sq.add_batch(None, x[i * n:(i + 1) * n].clone().unsqueeze(0))
    assert sq.nsamples == nsamples
    kw = dict(include_sparse=True, sparsity_threshold=0.99, nuq=True, fisher=None, norm=False, cap_outliers=False,
              first_few_fp16=-1)
    kw.update(qkw)
    if kw["fisher"] == "fisher":
        kw["fisher"] = fisher()
    with one_thread():
        return sq.quantize(**kw)


def main():
    ref = load_ref()
    out = {}
    for name in CASES:
        r = run_ref(ref, name)
        out[name + "_upper"] = np.asarray(r[0])
        out[name + "_lower"] = np.asarray(r[1])
        out[name + "_centroids"] = np.asarray(r[2][0])
    np.savez_compressed(GOLD, **out)
    print("wrote calibrate_ref.npz:", sorted(out))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    main()
