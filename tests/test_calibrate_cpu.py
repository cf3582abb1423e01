"""kvquant_amd.calibrate against the reference's SimQuant.quantize (its quantizer tuples for seeded activations are
stored in tests/golden/calibrate_ref.npz, made by tests/golden/gen_calibrate.py; both sides fit on one thread):
identical thresholds, the same k-means signposts; plus format / property checks."""
import numpy as np
import pytest
import torch

from kvquant_amd import calibrate
from tests.golden import gen_calibrate as gen

_data = gen.data


def _ref(name):
    g = np.load(gen.GOLD)
    return g[name + "_upper"], g[name + "_lower"], [g[name + "_centroids"]]


def test_quantizer_tuple_format_and_properties():
    x = _data()
    q = calibrate.calibrate_tensor(x, 3, True, 0.99, norm=True)
    up, lo, cent, ns, no = q
    assert up.shape == (1, 256) and lo.shape == (1, 256) and cent[0].shape == (8, 1)
    frac = float(((x > torch.tensor(up)) | (x < torch.tensor(lo))).float().mean())
    assert 0.005 < frac < 0.015                                # 1 % of the entries cross the thresholds
    c = np.sort(cent[0].flatten())
    assert -1.0 <= c[0] < c[-1] <= 1.0                         # signposts live in the normalised range
    assert 0.5 < float(ns) < 2.0 and abs(float(no)) < 0.5


@pytest.mark.parametrize("bits", [2, 4])
def test_matches_reference_simquant(bits):
    r = _ref("simquant_b%d" % bits)
    x = _data(seed=bits)
    with gen.one_thread():
        m = calibrate.calibrate_tensor(x, bits, True, 0.99)
    assert np.array_equal(np.asarray(r[0]).flatten(), m[0].flatten())
    assert np.array_equal(np.asarray(r[1]).flatten(), m[1].flatten())
    assert np.abs(np.sort(r[2][0].flatten()) - np.sort(m[2][0].flatten())).max() < 1e-4


def _same(r, m, tol=1e-4):
    assert np.array_equal(np.asarray(r[0]).flatten(), m[0].flatten())
    assert np.array_equal(np.asarray(r[1]).flatten(), m[1].flatten())
    assert np.abs(np.sort(r[2][0].flatten()) - np.sort(m[2][0].flatten())).max() < tol


def test_capped_outliers_and_sink_exclusion_match_reference():
    """SQ:421-461 + 441-446 / 487-491: the k-means mask of the capped-outlier K calibration with the first tokens of
    every sample excluded (the reference hard-codes 16 samples x 2048 tokens = 32768 rows)."""
    r = _ref("capped")
    x = _data(seed=5, T=32768, C=24)
    with gen.one_thread():
        m = calibrate.calibrate_tensor(x, 2, True, 0.99, cap_outliers=True, first_few_fp16=5, nsamples=16, seqlen=2048)
    _same(r, m)
    # the exclusion matters: without it the fit is a different one
    with gen.one_thread():
        m2 = calibrate.calibrate_tensor(x, 2, True, 0.99, cap_outliers=False, first_few_fp16=-1)
    assert np.abs(np.sort(m2[2][0].flatten()) - np.sort(m[2][0].flatten())).max() > 1e-6


def test_fisher_weighted_kmeans_matches_reference():
    """SQ:507-518: the squared-gradient weights enter the k-means fit as sample weights"""
    r = _ref("fisher")
    x = _data(seed=7, T=2048, C=64)
    fisher = gen.fisher()
    with gen.one_thread():
        m = calibrate.calibrate_tensor(x, 3, True, 0.99, fisher=fisher)
    _same(r, m)
    with gen.one_thread():
        plain = calibrate.calibrate_tensor(x, 3, True, 0.99)
    assert np.abs(np.sort(plain[2][0].flatten()) - np.sort(m[2][0].flatten())).max() > 1e-4


def test_value_pass_matches_reference():
    """llama_simquant.py:229-235: v_proj is calibrated with SimQuant(perchannel=True, qchannel=-1) -- per-token
    thresholds [T, 1], signposts from the per-token normalised values"""
    r = _ref("value")
    x = _data(seed=9, T=512, C=256)
    with gen.one_thread():
        m = calibrate.calibrate_tensor(x, 4, True, 0.99, qchannel=-1)
    assert m[0].shape == (512, 1)
    _same(r, m)


def test_subsampling_is_opt_in_and_reported():
    x = _data(seed=3, T=1024, C=64)
    msgs = []
    q = calibrate.calibrate_tensor(x, 2, True, 0.99, max_points=5000, log=msgs.append)
    assert len(msgs) == 1 and "subsample" in msgs[0] and q[2][0].shape == (4, 1)
    msgs.clear()
    calibrate.calibrate_tensor(x, 2, True, 0.99, log=msgs.append)
    assert not msgs


def test_nearest_is_chunked():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1000, 7, generator=g)
    poles = torch.tensor([-1.0, -0.2, 0.3, 0.9])
    a = calibrate._nearest(x, poles, chunk=333)
    b = poles[(x.reshape(1, -1) - poles.view(-1, 1)).abs().argmin(dim=0)].reshape(x.shape)
    assert torch.equal(a, b)
