"""CPU: the host side of the BOP errors - bop_average_recall on hand-built errors whose recalls are known, and
symmetry_tfs_from_info (src/Utils.py:806-835) on discrete and continuous BOP models_info entries."""
import numpy as np
import pytest

from foundationpose_amd import Utils as U


def test_thresholds():
  assert np.allclose(U.BOP19_VSD_TAUS, np.arange(1, 11) * 0.05) and len(U.BOP19_VSD_TAUS) == 10
  assert np.allclose(U.BOP19_VSD_THETAS, np.arange(1, 11) * 0.05) and np.allclose(U.BOP19_MSSD_THETAS, np.arange(1, 11) * 0.05)
  assert np.array_equal(U.BOP19_MSPD_THETAS, np.arange(5, 51, 5))
  assert U.BOP19_VSD_DELTA == 0.015


def test_average_recall_known_values():
  # MSSD with diameter 1: an error of 0.12 is below 8 of the 10 thresholds 0.05 .. 0.5, 0 below all, 0.6 below none
  r = U.bop_average_recall(e_mssd=[0.12, 0.0, 0.6], diameter=1.0)
  assert r == {'AR_MSSD': pytest.approx((8 + 10 + 0) / 30)}
  # strictly below: an error equal to a threshold misses it (0.05 is below 9 of them)
  assert U.bop_average_recall(e_mssd=[0.05], diameter=1.0)['AR_MSSD'] == pytest.approx(0.9)
  # MSPD in pixels at 640 wide: 12 px is below 8 of 5 .. 50; at 1280 wide the thresholds double, 12 px is below 9 of 10 .. 100
  assert U.bop_average_recall(e_mspd=[12.0])['AR_MSPD'] == pytest.approx(0.8)
  assert U.bop_average_recall(e_mspd=[12.0], image_width=1280)['AR_MSPD'] == pytest.approx(0.9)
  # VSD: every (tau, theta) pair; an estimate whose e is 0.3 at every tau is correct for theta 0.35 .. 0.5 (4 of 10)
  e = np.full((2, 10), 0.3)
  e[1] = 1.0
  assert U.bop_average_recall(e_vsd=e)['AR_VSD'] == pytest.approx(4 / 20)
  # e depending on tau: correct for every theta at the first 5 taus, for none at the last 5
  e = np.concatenate([np.zeros(5), np.ones(5)])[None]
  assert U.bop_average_recall(e_vsd=e)['AR_VSD'] == pytest.approx(0.5)


def test_average_recall_all_three_and_missing_targets():
  e_vsd = np.zeros((3, 10))
  r = U.bop_average_recall(e_vsd=e_vsd, e_mssd=[0.0, 0.0, 1.0], e_mspd=[1.0, 100.0, 3.0], diameter=0.1)
  assert r['AR_VSD'] == 1.0 and r['AR_MSSD'] == pytest.approx(2 / 3) and r['AR_MSPD'] == pytest.approx(2 / 3)
  assert r['AR'] == pytest.approx((1 + 2 / 3 + 2 / 3) / 3)
  # two targets have no estimate: they count as misses
  r = U.bop_average_recall(e_vsd=e_vsd, e_mssd=[0.0, 0.0, 1.0], e_mspd=[1.0, 100.0, 3.0], diameter=0.1, n_targets=5)
  assert r['AR_VSD'] == pytest.approx(3 / 5) and r['AR_MSSD'] == pytest.approx(2 / 5) and r['AR_MSPD'] == pytest.approx(2 / 5)
  assert r['AR'] == pytest.approx((3 + 2 + 2) / 15)
  with pytest.raises(ValueError):
    U.bop_average_recall(e_mssd=[0.0, 0.0], diameter=0.1, n_targets=1)
  with pytest.raises(ValueError):
    U.bop_average_recall(e_mssd=[0.0])                                 # no diameter
  with pytest.raises(ValueError):
    U.bop_average_recall()


def test_average_recall_per_target_diameter():
  # the same error 0.032 m against a 0.1 m object (below 0.035 .. 0.05 of the thresholds 0.005 .. 0.05: 4 of 10) and a 1 m object (all 10)
  r = U.bop_average_recall(e_mssd=[0.032, 0.032], diameter=[0.1, 1.0])
  assert r['AR_MSSD'] == pytest.approx((4 + 10) / 20)
  r = U.bop_average_recall(e_mssd=np.array([0.3, 0.3]), diameter=np.array([1.0, 0.1]))
  assert r['AR_MSSD'] == pytest.approx((4 + 0) / 20)


def test_symmetry_tfs_discrete():
  R = np.diag([-1.0, -1.0, 1.0])
  tf1 = np.eye(4)
  tf1[:3, :3] = R
  tf1[:3, 3] = [0.0, 0.0, 12.0]                                       # millimetres, as in models_info
  tf2 = np.eye(4)
  tf2[:3, :3] = np.diag([1.0, -1.0, -1.0])
  info = {'symmetries_discrete': [tf1.reshape(-1).tolist(), tf2.reshape(-1).tolist()]}
  out = U.symmetry_tfs_from_info(info)
  assert out.shape == (3, 4, 4)
  assert np.array_equal(out[0], np.eye(4))
  assert np.allclose(out[1][:3, 3], [0, 0, 0.012]) and np.array_equal(out[1][:3, :3], R)
  assert np.array_equal(out[2], tf2)
  for T in out:
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3)) and np.array_equal(T[3], [0, 0, 0, 1])


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_symmetry_tfs_continuous(axis):
  ax = [0, 0, 0]
  ax[axis] = 1
  info = {'symmetries_continuous': [{'axis': ax, 'offset': [1.0, 2.0, 3.0]}]}
  out = U.symmetry_tfs_from_info(info)
  assert out.shape == (1 + 72, 4, 4)                                 # the identity twice: first, and as the 0-degree rotation
  assert np.array_equal(out[0], np.eye(4))
  assert np.array_equal(out[1][:3, :3], np.eye(3))
  assert np.array_equal(out[1:, :3, 3], np.tile([1.0, 2.0, 3.0], (72, 1)))      # the offset is not scaled
  for T in out:
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(T[:3, :3]), 1)
    assert np.allclose(T[:3, :3][:, axis], np.eye(3)[axis])          # a rotation about that axis
  ang = np.arctan2(out[2][(axis + 2) % 3, (axis + 1) % 3], out[2][(axis + 1) % 3, (axis + 1) % 3])
  assert np.isclose(ang, np.deg2rad(5))
  assert U.symmetry_tfs_from_info(info, rot_angle_discrete=90).shape == (5, 4, 4)


def test_symmetry_tfs_both_and_none():
  tf = np.eye(4)
  tf[:3, :3] = np.diag([1.0, -1.0, -1.0])
  info = {'symmetries_discrete': [tf.reshape(-1).tolist()], 'symmetries_continuous': [{'axis': [0, 0, 1], 'offset': [0, 0, 0]}]}
  assert U.symmetry_tfs_from_info(info).shape == (2 + 72, 4, 4)
  assert np.array_equal(U.symmetry_tfs_from_info({'diameter': 100.0}), np.eye(4)[None])
