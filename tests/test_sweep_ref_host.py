"""The exact family of tests/_sweep_ref.py, proven on the host (no GPU): the numpy model of the blocked symmetric sweep of
csrc/linalg.hip returns the closed-form integer inverse exactly, at both pivot-block widths, plain and scaled by powers of two;
its intermediates stay far below 2^53 (cap 2^20: the condition under which tests/test_gpu_factor_exact.py may demand bit-exact
results from the device, not a measurement); a planted negative pivot is met exactly where it was planted."""
import functools

import numpy as np
import pytest

import _sweep_ref as R

SIZES = [200, 640, 1000, 1100, 2100]


@functools.lru_cache(maxsize=None)
def clean_sweep(n, nb):
    return R.blocked_sweep(R.unimodular_spd(n)[0], nb)


@pytest.mark.parametrize("nb", [64, 128])
@pytest.mark.parametrize("n", SIZES)
def test_model_returns_the_closed_form_inverse_exactly(n, nb):
    H, Hinv = R.unimodular_spd(n)
    M, big, bad = clean_sweep(n, nb)
    assert bad is None
    assert np.array_equal(M, Hinv), R.first_mismatch(M, Hinv, nb)
    assert big < R.CAP, np.log2(big)
    q = -(-n // 64) * 64                                           # no 64 x 64 block of the inverse is all zero: every tile of every update matters
    Z = np.zeros((q, q)); Z[:n, :n] = Hinv
    assert (np.abs(Z).reshape(q // 64, 64, q // 64, 64).max(axis=(1, 3)) > 0).all()


@pytest.mark.parametrize("nb", [64, 128])
@pytest.mark.parametrize("n", SIZES)
def test_model_is_exact_on_the_power_of_two_scaling(n, nb):
    H, Hinv = R.unimodular_spd(n)
    Hs, His, D = R.scaled(H, Hinv)
    assert np.array_equal(Hs / D[:, None] / D[None, :], H) and np.array_equal(His * D[:, None] * D[None, :], Hinv)   # the scaling itself is exact
    ex = np.log2(np.abs(His[His != 0]))
    assert ex.max() - ex.min() > 60                                # entries spread over many decades
    M, big, bad = R.blocked_sweep(Hs, nb, D)
    assert bad is None
    assert np.array_equal(M, His), R.first_mismatch(M, His, nb)
    assert big < R.CAP, np.log2(big)                               # (in the units of the unscaled matrix)
    assert big == clean_sweep(n, nb)[1]                            # the same integers, shifted


def test_the_generator_is_cached_and_read_only():
    H, Hinv = R.unimodular_spd(200)
    assert R.unimodular_spd(200)[0] is H and not H.flags.writeable and not Hinv.flags.writeable
    H2, _ = R.unimodular_spd(200, seed=1)
    assert not np.array_equal(H, H2)
    assert np.array_equal(np.linalg.eigvalsh(H) > 0, np.ones(200, bool))


@pytest.mark.parametrize("n", [1100, 2300])
def test_a_planted_negative_pivot_is_met_exactly_there(n):
    H, _ = R.unimodular_spd(n)
    for j in (0, 127, 128 * 3 + 5, n - 1):
        for nb in (64, 128):
            M, big, bad = R.blocked_sweep(R.plant_negative_pivot(H, j), nb, stop_at_bad=True)
            assert bad == j, (j, nb, bad)                          # d <= 0 at pivot j and not before
    for j in (0, 128 * 3 + 5) if n == 1100 else ():                # swept to the end: everything after the bad pivot stays finite
        M, big, bad = R.blocked_sweep(R.plant_negative_pivot(H, j), 128)
        assert bad == j and np.isfinite(M).all() and np.isfinite(big)


@pytest.mark.parametrize("n", [200, 1000, 1100])
def test_padding_with_the_identity_pads_the_inverse(n):
    H, Hinv = R.unimodular_spd(n)
    q = R.padded_size(n)
    assert q % 128 == 0 and 0 <= q - n < 128
    M, big, bad = R.blocked_sweep(R.pad_identity(H, q), 128)
    assert bad is None and big < R.CAP
    assert np.array_equal(M, R.pad_identity(Hinv, q))


def test_knob_sets_extend_the_existing_list():
    assert len(R.KNOB_SETS) == 19 and R.KNOB_SETS[0] == {}
    assert R.KNOB_SETS[-2] == {"LPVS_FACTOR_GROUP": "4", "LPVS_RU_STAGE": "8", "LPVS_PIVOT_ALONE": "0"}
    assert R.KNOB_SETS[-1] == dict(R.KNOB_SETS[-2], LPVS_BAND_TILE="128")
    assert len({R.knob_id(k) for k in R.KNOB_SETS}) == len(R.KNOB_SETS)
