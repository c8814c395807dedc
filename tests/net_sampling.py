"""Shared by the GPU tests of the network families' sampling rule (test_gpu_net_s16_family.py,
test_gpu_net_s25_family.py): the check of a sample's probability product."""
import numpy as np


def check_pp(name, pp, want, n_steps):
    """pp float32 against the float64 product ``want`` of a sample's n_steps probabilities: rtol = 1e-5 wherever float32
    holds the product as a normal number.  Below its smallest normal number (1.18e-38; at wide16 48 probabilities of 8
    logits come to about 1e-40) float32 is subnormal, with an absolute spacing of 2^-149 and no relative precision to
    speak of: each multiply of the running product then rounds by up to half a spacing, and the later factors, all
    below 1, only shrink the earlier roundings, so n_steps / 2 spacings bound their sum.  Only there is that added."""
    tiny = float(np.finfo(np.float32).tiny)
    sub = want < tiny
    print(f"{name}: {int(sub.sum())} of {sub.size} products are subnormal in float32")
    assert np.isfinite(pp).all() and (pp >= 0).all()
    bound = 1e-5 * np.abs(want) + np.where(sub, 0.5 * n_steps * 2.0 ** -149, 0.0)
    bad = np.abs(pp.astype(np.float64) - want) > bound
    assert not bad.any(), (name, pp[bad][:4], want[bad][:4])
