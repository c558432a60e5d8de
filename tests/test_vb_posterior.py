"""The helper of the online VB lists' tests (tests/vb_posterior.py) held to exact arithmetic and to
its own claims, and the posterior file against sbmf_vb_posterior_file_info -- no GPU.

  * moments on the exact construction equals fractions.Fraction;
  * the guests' inputs (smooth_state) are such that 64 scans reach the fixed point A m = c to 1e-12
    relative, and no scan moves the longdouble restatement away from it;
  * a numpy-written file reads back through the library's header reader; a truncated file, a wrong
    magic and the other malformed headers are refused."""
import struct

import numpy as np
import pytest

import sbmf
from vb_posterior import (MAGIC, exact_state, file_bytes, guest_limit, guest_scan, make_guests, moments, moments_fraction,
                          smooth_state, write_posterior)

GUEST_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)
GUEST_KS = (1, 16, 17, 100, 200)
GUEST_J = 1100


@pytest.mark.parametrize("K", [1, 7, 16, 33])
def test_moments_equal_fractions_on_the_exact_construction(K):
    st = exact_state(9, 21, K, 5)
    for a in ("Um", "Vm", "bum", "bvm"):
        assert np.all(st[a] * 4 == np.round(st[a] * 4)) and np.abs(st[a]).max() <= 2
    for a in ("Us", "Vs", "bus", "bvs", "sigma_v"):
        assert np.all(st[a] * 4 == np.round(st[a] * 4)) and st[a].min() >= 0.25 and st[a].max() <= 2
    mean, var = moments(st, np.arange(9))
    assert var.max() < 20 * K + 6
    for u in range(9):
        for j in range(21):
            fm, fv = moments_fraction(st, u, j)
            assert fm == mean[u, j] and float(fm) == mean[u, j]
            assert fv == var[u, j] and float(fv) == var[u, j]
    # a permuted summation order gives the same bits: the sums are exact
    p = np.random.default_rng(1).permutation(K)
    st2 = dict(st, Um=st["Um"][:, p], Us=st["Us"][:, p], Vm=st["Vm"][:, p], Vs=st["Vs"][:, p])
    m2, v2 = moments(st2, np.arange(9))
    assert np.array_equal(m2, mean) and np.array_equal(v2, var)


@pytest.mark.parametrize("K", GUEST_KS)
def test_guest_inputs_converge_to_the_limit(K):
    st = smooth_state(4, GUEST_J, K, 77)
    guests = make_guests(GUEST_J, GUEST_LENGTHS, K)
    g64, var, b64, bvar = guest_scan(st, guests, 64)
    worst = 0.0
    for q, (it, r) in enumerate(guests):
        bl, gl = guest_limit(st, it, r)
        lim, got = np.concatenate([[bl], gl]), np.concatenate([[b64[q]], g64[q]])
        rel = np.abs(got - lim).max() / max(np.abs(lim).max(), 1e-300)
        worst = max(worst, rel)
        assert rel <= 1e-12, (K, len(it), rel)
        if len(it) == 0:  # the prior exactly
            assert not got.any() and np.array_equal(var[q], 1 / st["sigma_v"]) and bvar[q] == 1 / st["sigma_w"]
    print("K=%d: largest relative distance of 64 scans from the limit %.3g" % (K, worst))
    assert np.all(var > 0) and np.all(bvar > 0)


def test_a_scan_never_moves_away_from_the_limit():
    K = 17
    st = smooth_state(4, GUEST_J, K, 77)
    guests = make_guests(GUEST_J, (1, 5, 64, 257), K)
    trace = []
    guest_scan(st, guests, 12, np.longdouble, trace)
    A_dist = []
    for b, g in trace:
        d = []
        for q, (it, r) in enumerate(guests):
            bl, gl = guest_limit(st, it, r)
            d.append(float(max(abs(b[q] - bl), np.abs(g[q] - gl).max())))
        A_dist.append(d)
    A_dist = np.array(A_dist)
    floor = 1e-13  # the limit itself is a float64 solve
    assert np.all((A_dist[1:] <= A_dist[:-1]) | (A_dist[1:] < floor)), A_dist


def test_float64_and_longdouble_restatements_agree_closely():
    st = smooth_state(4, GUEST_J, 16, 77)
    guests = make_guests(GUEST_J, (3, 65), 16)
    a, b = guest_scan(st, guests, 2), guest_scan(st, guests, 2, np.longdouble)
    for x, y in zip(a, b):
        assert np.allclose(x, np.asarray(y, np.float64), rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------ the file
@pytest.mark.parametrize("I,J,K", [(1, 1, 1), (5, 9, 3), (131, 261, 17), (3, 2, 256)])
def test_file_round_trip_against_file_info(tmp_path, I, J, K):
    p = tmp_path / "post.vb"
    write_posterior(p, exact_state(I, J, K, 3))
    assert p.stat().st_size == file_bytes(I, J, K)
    assert sbmf.vb_posterior_file_info(p) == {"version": 1, "num_users": I, "num_items": J, "num_factor": K,
                                              "bytes": file_bytes(I, J, K)}


def _refused(tmp_path, data):
    p = tmp_path / "bad.vb"
    p.write_bytes(data)
    with pytest.raises(sbmf.SBMFError) as ei:
        sbmf.vb_posterior_file_info(p)
    assert ei.value.code == sbmf.SBMF_E_IO
    return str(ei.value)


def test_malformed_files_are_refused(tmp_path):
    p = tmp_path / "post.vb"
    write_posterior(p, exact_state(5, 9, 3, 3))
    good = p.read_bytes()
    assert "bad magic" in _refused(tmp_path, b"SBMFSMP\n" + good[8:])
    assert "truncated in its header" in _refused(tmp_path, good[:23])
    assert "truncated in its body" in _refused(tmp_path, good[:-1])
    assert "truncated in its body" in _refused(tmp_path, good[:24])
    assert "trailing bytes" in _refused(tmp_path, good + b"\0")
    assert "version 2" in _refused(tmp_path, MAGIC + struct.pack("<4I", 2, 5, 9, 3) + good[24:])
    assert "bad field" in _refused(tmp_path, MAGIC + struct.pack("<4I", 1, 5, 9, 0) + good[24:])
    assert "bad field" in _refused(tmp_path, MAGIC + struct.pack("<4I", 1, 5, 9, 257) + good[24:])
    with pytest.raises(sbmf.SBMFError) as ei:
        sbmf.vb_posterior_file_info(tmp_path / "missing")
    assert ei.value.code == sbmf.SBMF_E_IO and "cannot open" in str(ei.value)
