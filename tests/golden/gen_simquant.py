"""Generates tests/golden/simquant_ref.npz from the reference's OWN simulated-quantisation functions
(/root/reference/quant/kvquant/simquant_module_quantizer.py imported here; nothing is copied):
seeded inputs -> get_outliers / get_outliers_dynamic / quant_fn_nuq_recon outputs for the K (per-channel,
static thresholds, capped outliers) and V (per-token, dynamic) configurations at 2, 3 and 4 bit; and
tests/golden/simquant_wrappers_ref.npz: the same functions at 4 bit with first-token exclusion and with the argument
plumbing of QuantLinearSim.forward, on a longer input.
Run in the build container:  python tests/golden/gen_simquant.py"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/quant/kvquant/simquant_module_quantizer.py"
WRAPPERS = os.path.join(HERE, "simquant_wrappers_ref.npz")


def load_ref():
    spec = importlib.util.spec_from_file_location("ref_simquant", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def inputs(bits, T=24, C=256, seed=0):
    g = torch.Generator().manual_seed(seed + bits)
    scale = torch.exp(0.5 * torch.randn(C, generator=g))
    shift = 0.3 * torch.randn(C, generator=g)
    k = (torch.randn(T, C, generator=g) * scale + shift)
    k[torch.rand(T, C, generator=g) < 0.02] *= 4.0
    v = torch.randn(T, C, generator=g)
    v[torch.rand(T, C, generator=g) < 0.02] *= 5.0
    up = (shift + 2.4 * scale).half()
    lo = (shift - 2.4 * scale).half()
    n = 2 ** bits
    cent = torch.sort(torch.rand(n, generator=g) * 2 - 1).values.numpy().reshape(n, 1)
    return k.half().float(), v.half().float(), up, lo, [cent]


def main():
    ref = load_ref()
    out = {}
    for bits in (2, 3, 4):
        k, v, up, lo, lut = inputs(bits)
        mk = ref.get_outliers(k, channel=0, outlier_threshold_upper=up, outlier_threshold_lower=lo, cap_outliers=21,
                              first_few_fp16=-1)
        qk = ref.quant_fn_nuq_recon(k, bits=bits, qchannel=0, maxval=up, minval=lo, include_sparse=True,
                                    outlier_mask=mk, dynamicquantization=False, lut=lut)
        mv = ref.get_outliers_dynamic(v, channel=-1, thresh=0.99, first_few_fp16=2)
        qv = ref.quant_fn_nuq_recon(v, bits=bits, qchannel=-1, include_sparse=True, outlier_mask=mv,
                                    dynamicquantization=True, lut=lut, first_few_fp16=2)
        qn = ref.quant_fn_nuq_recon(k, bits=bits, qchannel=0, maxval=up, minval=lo, include_sparse=True,
                                    outlier_mask=mk, dynamicquantization=False, lut=lut, norm=True,
                                    normscale=torch.tensor(1.05), normoffset=torch.tensor(-0.01))
        for name, t in (("mk", mk), ("qk", qk), ("mv", mv), ("qv", qv), ("qn", qn)):
            out["b%d_%s" % (bits, name)] = t.numpy()
    np.savez_compressed(os.path.join(HERE, "simquant_ref.npz"), **out)
    print("wrote simquant_ref.npz:", sorted(out))
    out = wrappers(ref)
    np.savez_compressed(WRAPPERS, **out)
    print("wrote simquant_wrappers_ref.npz:", sorted(out))


def wrapper_inputs(T=40, C=512, seed=11):
    """inputs() at 4 bit, drawn in float64 by numpy's PCG64 with correctly rounded arithmetic only and rounded once:
    the same bits on every CPU (torch's vectorised randn / exp depend on the CPU's instruction set)"""
    rng = np.random.default_rng(seed)
    scale = rng.lognormal(0.0, 0.5, C)
    shift = 0.3 * rng.standard_normal(C)
    k = rng.standard_normal((T, C)) * scale + shift
    k[rng.random((T, C)) < 0.02] *= 4.0
    v = rng.standard_normal((T, C))
    v[rng.random((T, C)) < 0.02] *= 5.0
    up = torch.from_numpy((shift + 2.4 * scale).astype(np.float16))
    lo = torch.from_numpy((shift - 2.4 * scale).astype(np.float16))
    cent = np.sort(rng.random(16) * 2 - 1).astype(np.float32).reshape(16, 1)
    return (torch.from_numpy(k.astype(np.float16)).float(), torch.from_numpy(v.astype(np.float16)).float(), up, lo,
            [cent])


def wrappers(ref):
    """4 bit, first 3 tokens kept in fp16 (mk3 / q3); the K and V calls of QuantLinearSim.forward (SQ:700-795) without
    that exclusion (qk, qv)"""
    k, v, up, lo, lut = wrapper_inputs()
    mk3 = ref.get_outliers(k, channel=0, outlier_threshold_upper=up, outlier_threshold_lower=lo, cap_outliers=21,
                           first_few_fp16=3)
    q3 = ref.quant_fn_nuq_recon(k, bits=4, qchannel=0, maxval=up, minval=lo, include_sparse=True, outlier_mask=mk3,
                                lut=lut, first_few_fp16=3)
    mk = ref.get_outliers(k, channel=0, outlier_threshold_upper=up, outlier_threshold_lower=lo, cap_outliers=21)
    qk = ref.quant_fn_nuq_recon(k, bits=4, qchannel=0, maxval=up, minval=lo, include_sparse=True, outlier_mask=mk,
                                lut=lut)
    mv = ref.get_outliers_dynamic(v, channel=-1, thresh=0.99)
    qv = ref.quant_fn_nuq_recon(v, bits=4, qchannel=-1, include_sparse=True, outlier_mask=mv, dynamicquantization=True,
                                lut=lut)
    return {name: t.numpy() for name, t in (("mk3", mk3), ("q3", q3), ("qk", qk), ("qv", qv))}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    main()
