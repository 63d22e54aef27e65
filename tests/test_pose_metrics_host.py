"""CPU: compute_auc_sklearn (src/Utils.py:255-267) on the host - against a numpy restatement of the reference's loop, against
sklearn.metrics.auc where sklearn is installed, and on cases whose area is known."""
import numpy as np
import pytest

from foundationpose_amd import Utils as U

_trapezoid = getattr(np, 'trapezoid', None) or np.trapz


def auc_restated(errs, max_val=0.1, step=0.001):
  errs = np.sort(np.array(errs))
  X = np.arange(0, max_val + step, step)
  Y = np.ones(len(X))
  for i, x in enumerate(X):
    y = (errs <= x).sum() / len(errs)
    Y[i] = y
    if y >= 1:
      break
  return X, Y, _trapezoid(Y, X) / max_val


CASES = [
  (np.random.RandomState(0).uniform(0, 0.15, 500), 0.1, 0.001),
  (np.random.RandomState(1).exponential(0.02, 252), 0.1, 0.001),
  (np.random.RandomState(2).uniform(0, 0.04, 33), 0.1, 0.001),       # every error covered early: the curve's early break
  (np.random.RandomState(3).uniform(0, 0.3, 1000), 0.2, 0.005),
  ([0.01, 0.02, 0.5], 0.05, 0.01),
]


@pytest.mark.parametrize('errs,max_val,step', CASES)
def test_auc_matches_the_reference_loop(errs, max_val, step):
  got = U.compute_auc_sklearn(errs, max_val=max_val, step=step)
  assert isinstance(got, float)
  assert got == pytest.approx(auc_restated(errs, max_val, step)[2], rel=0, abs=1e-12)


@pytest.mark.parametrize('errs,max_val,step', CASES)
def test_auc_matches_sklearn(errs, max_val, step):
  metrics = pytest.importorskip('sklearn.metrics')
  X, Y, _ = auc_restated(errs, max_val, step)
  assert U.compute_auc_sklearn(errs, max_val=max_val, step=step) == pytest.approx(metrics.auc(X, Y) / max_val, rel=0, abs=1e-12)


def test_auc_known_areas():
  assert U.compute_auc_sklearn(np.zeros(10)) == pytest.approx(1.0, abs=1e-12)
  assert U.compute_auc_sklearn(np.full(7, 0.5)) == 0.0
  # half the errors at 0, half above max_val: y = 0.5 everywhere -> area 0.5
  assert U.compute_auc_sklearn([0.0, 0.0, 1.0, 1.0]) == pytest.approx(0.5, abs=1e-12)
  # one step: y = 0 up to x = 0.05 - step, 1 from x = 0.05 (grid 0, 0.01, .., 0.1): trapezoid area = 0.05 + 0.01 / 2
  assert U.compute_auc_sklearn([0.045], max_val=0.1, step=0.01) == pytest.approx((0.05 + 0.005) / 0.1, abs=1e-12)


def test_product_does_not_import_sklearn():
  import inspect
  src = inspect.getsource(U)
  assert 'import sklearn' not in src and 'from sklearn' not in src
