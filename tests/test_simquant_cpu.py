"""oracle/simquant.py (restatement of the reference's simulated-quantisation functions) against the reference:
bit-exact vs tests/golden/simquant_ref.npz and tests/golden/simquant_wrappers_ref.npz (made by the reference's own
module, tests/golden/gen_simquant.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import simquant as sq
from tests.golden import gen_simquant as gen

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simquant_ref.npz")


def _ours(bits):
    k, v, up, lo, lut = gen.inputs(bits)
    mk = sq.get_outliers(k, channel=0, outlier_threshold_upper=up, outlier_threshold_lower=lo, cap_outliers=21)
    qk = sq.quant_fn_nuq_recon(k, bits=bits, qchannel=0, maxval=up, minval=lo, include_sparse=True, outlier_mask=mk, lut=lut)
    mv = sq.get_outliers_dynamic(v, channel=-1, thresh=0.99, first_few_fp16=2)
    qv = sq.quant_fn_nuq_recon(v, bits=bits, qchannel=-1, include_sparse=True, outlier_mask=mv, dynamicquantization=True,
                               lut=lut, first_few_fp16=2)
    qn = sq.quant_fn_nuq_recon(k, bits=bits, qchannel=0, maxval=up, minval=lo, include_sparse=True, outlier_mask=mk, lut=lut,
                               norm=True, normscale=torch.tensor(1.05), normoffset=torch.tensor(-0.01))
    return dict(mk=mk, qk=qk, mv=mv, qv=qv, qn=qn)


@pytest.mark.parametrize("bits", [2, 3, 4])
def test_simquant_matches_reference_golden(bits):
    g = np.load(GOLD)
    for name, t in _ours(bits).items():
        ref = g["b%d_%s" % (bits, name)]
        assert np.array_equal(t.numpy(), ref), name


def test_simquant_matches_reference_live():
    """first-token exclusion and the QuantLinearSim.forward argument plumbing (SQ:700-795) on a longer input, vs the
    reference's outputs stored in tests/golden/simquant_wrappers_ref.npz"""
    g = np.load(gen.WRAPPERS)
    k, v, up, lo, lut = gen.wrapper_inputs()
    mk = sq.get_outliers(k, channel=0, outlier_threshold_upper=up, outlier_threshold_lower=lo, cap_outliers=21,
                         first_few_fp16=3)
    assert np.array_equal(mk.numpy(), g["mk3"])
    b = sq.quant_fn_nuq_recon(k, bits=4, qchannel=0, maxval=up, minval=lo, include_sparse=True, outlier_mask=mk, lut=lut,
                              first_few_fp16=3)
    assert np.array_equal(b.numpy(), g["q3"])
    quant = (up.float().numpy()[None], lo.float().numpy()[None], lut)
    # the wrappers reproduce QuantLinearSim.forward's argument plumbing (SQ:700-795)
    assert torch.equal(sq.fake_quant_k(k, quant, 4, cap_outliers=21), torch.from_numpy(g["qk"]).half())
    assert torch.equal(sq.fake_quant_v(v, quant, 4, sparsity_threshold=0.99), torch.from_numpy(g["qv"]).half())
