"""What every transform of an uneven record answers to a record it cannot take (csrc/uneven.hip: Record::check, after the scan of lomb.hip):
the exception type and the WHOLE message, for the six Python entry points and every fault of the list below.  "Not finite" wins over
"negative", "negative" over the rule for the sum of the weights; the prefix is the family's.  Weights that are all zero are refused where
the sum normalises them (lombscargle, its several-harmonic and bootstrap forms, bls) and taken where every cell or window forms its own sum
(wwz, the windowed forms: everything comes back empty).  Two signals, N = 600: three blocks of the scan, the last one partial, with the
faults in the first and in the last.  GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NS = 600, 2
NOT_FINITE = "{}: t, y or W holds a value that is not finite"
NEGATIVE = "{}: a weight is negative"
ZERO_SUM = "{}: the weights sum to 0"
NOT_SORTED = "{}: t is not sorted (it decreases somewhere)"
EMPTY = "taken: everything empty"


def _record():
    rng = np.random.default_rng(600)
    t = np.sort(rng.integers(0, 40 * 1024, N)) / 1024.0
    y = np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(NS)[None, :]) + 0.5 * rng.standard_normal((N, NS)) + 0.75
    return t, y, rng.uniform(0.5, 2.0, N)


F = np.arange(16, 48) / 64.0
TAU = np.array([5.0, 20.0, 35.0])
WINDOWS = (np.array([0, 200, 400], dtype=np.int64), np.array([200, 200, 200], dtype=np.int64), np.array([-1.0, 10.0, 25.0]), np.array([15.0, 30.0, 41.0]))

# name -> (the call, the prefix of its messages, its answer to weights that are all zero)
ENTRY = {
    "lombscargle": (lambda L, t, y, W: L.lombscargle(y, t, F, W=W, path="direct"), "lombscargle", ZERO_SUM),
    "lombscargle-nterms2": (lambda L, t, y, W: L.lombscargle(y, t, F, W=W, nterms=2), "lombscargle", ZERO_SUM),
    "lombscargle_spectrogram": (lambda L, t, y, W: L.lombscargle_spectrogram(y, t, F, windows=WINDOWS, W=W), "lombscargle", EMPTY),
    "wwz": (lambda L, t, y, W: L.wwz(y, t, F, tau=TAU, W=W), "wwz", EMPTY),
    "bls": (lambda L, t, y, W: L.bls(y, t, F, W=W, nbins=50), "bls", ZERO_SUM),
    "lombscargle_bootstrap": (lambda L, t, y, W: L.lombscargle_bootstrap(y[:, 1], t, F, W=W, B=8, seed=1), "lombscargle", ZERO_SUM),   # (one signal: the second)
}


def _nan_in_t(t, y, W):
    t[N - 1] = np.nan


def _inf_in_y(t, y, W):
    y[0, 1] = np.inf


def _nan_in_w(t, y, W):
    W[300] = np.nan


def _negative_weight(t, y, W):
    W[599] = -0.5


def _zero_weights(t, y, W):
    W[:] = 0.0


def _nan_and_negative_weight(t, y, W):
    W[0] = -1.0
    y[N - 1, 1] = np.nan                                                     # (the second signal: the one the bootstrap is given)


def _t_decreases(t, y, W):
    t[[100, 101]] = t[[101, 100]]
    assert t[100] > t[101]


# fault -> (what it does to the record, the message it draws; None: the entry's own answer to zero weights)
FAULTS = {
    "nan-in-t-at-599": (_nan_in_t, NOT_FINITE),
    "inf-in-second-signal-at-0": (_inf_in_y, NOT_FINITE),
    "nan-in-W": (_nan_in_w, NOT_FINITE),
    "negative-weight": (_negative_weight, NEGATIVE),
    "zero-weights": (_zero_weights, None),
    "nan-and-negative-weight": (_nan_and_negative_weight, NOT_FINITE),
}
CASES = [(e, k) for e in ENTRY for k in FAULTS] + [("wwz", "t-decreases")]


@pytest.mark.parametrize("entry,fault", CASES)
def test_refusal(L, entry, fault):
    call, prefix, zero = ENTRY[entry]
    spoil, message = (_t_decreases, NOT_SORTED) if fault == "t-decreases" else FAULTS[fault]
    message = zero if message is None else message
    t, y, W = _record()
    call(L, t, y, W)                                                         # the record itself is taken
    spoil(t, y, W)
    if message == EMPTY:
        r = call(L, t, y, W)
        assert r.empty.all() and not r.power.any()
        return
    with pytest.raises(ValueError) as e:
        call(L, t, y, W)
    assert str(e.value) == message.format(prefix)
