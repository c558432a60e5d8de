"""tests/sample_files.py without a GPU: the file it writes is the library's format, its reference
order is the plain tuple order, every family of the selection edge set has the property it exists
for, and its moments equal exact rational arithmetic on the exact constructions."""
import os
from fractions import Fraction

import numpy as np
import pytest

import sbmf
from sample_files import (FAMILY_RISKS, HIGH_RUNS, TINY, ZERO_BLOCK, expected_topn, key_families, key_image, moments,
                          rated_kinds, write_samples)

SEED = 20
TOPNS = (1, 2, 1023, 1024)


# ---- 1. the file header
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_file_is_what_the_library_reads(tmp_path, precision, bias, S):
    I, J, K = 5, 7, 3
    rng = np.random.default_rng(1)
    U, V = rng.integers(-8, 9, (S, I, K)) / 4.0, rng.integers(-8, 9, (S, J, K)) / 4.0
    kw = dict(b0=rng.integers(-4, 5, S) / 4.0, bu=rng.integers(-4, 5, (S, I)) / 4.0, bv=rng.integers(-4, 5, (S, J)) / 4.0) if bias else {}
    path = tmp_path / "hand.samples"
    write_samples(path, U, V, precision, sweeps=np.arange(S) * 2 + 1, **kw)
    ts = 4 if precision == "f32" else 8
    size = 40 + 4 * S + S * ((I + J) * K * ts + (8 * (1 + I + J) if bias else 0))
    assert os.path.getsize(path) == size
    assert sbmf.samples_file_info(path) == {"version": 1, "precision": precision, "num_users": I, "num_items": J,
                                            "num_factor": K, "count": S, "bias": bias, "bytes": size}
    # the body, read back by position: the sweeps, then the first sample's U
    raw = open(path, "rb").read()
    assert np.array_equal(np.frombuffer(raw, "<u4", S, 40), np.arange(S) * 2 + 1)
    ft = "<f4" if precision == "f32" else "<f8"
    assert np.array_equal(np.frombuffer(raw, ft, I * K, 40 + 4 * S).reshape(I, K), U[0])
    assert np.array_equal(np.frombuffer(raw, ft, J * K, size - (8 * (1 + I + J) if bias else 0) - J * K * ts).reshape(J, K), V[-1])
    if bias:
        assert np.array_equal(np.frombuffer(raw, "<f8", J, size - 8 * J), kw["bv"][-1])


def test_a_wrong_size_is_refused(tmp_path):
    path = tmp_path / "hand.samples"
    write_samples(path, np.ones((1, 2, 1)), np.ones((1, 3, 1)), "f64")
    with open(path, "ab") as f:
        f.write(b"\0")
    with pytest.raises(sbmf.SBMFError) as ei:
        sbmf.samples_file_info(path)
    assert "trailing" in str(ei.value)


# ---- 2. the reference order is the tuple order
def rows_of(J):
    """(name, sign, risk, mean, sd) of every family at J, for both kinds of user"""
    for name, sc in key_families(J, SEED).items():
        for sign in (1.0, -1.0):
            mean, _, sd = moments(sign * sc)
            for risk in FAMILY_RISKS.get(name, (0.0,)):
                yield name, sign, risk, mean, sd


@pytest.mark.parametrize("J", [300, 700])
def test_reference_order_is_the_tuple_order(J):
    rated = rated_kinds(J, SEED)
    seen = set()
    for name, sign, risk, mean, sd in rows_of(J):
        seen.add(name)
        key = mean - risk * sd
        for kind, r in rated:
            gone = set(r.tolist())
            # -k + 0.0: -0.0 and +0.0 are one key, as watch_key has it
            plain = [j for _, j in sorted((-float(key[j]) + 0.0, j) for j in range(J) if j not in gone)]
            for topn in (1, 2, 10, 1024):
                want = (plain + [-1] * topn)[:topn]
                assert expected_topn(mean, sd, r, topn, risk, True).tolist() == want, (name, sign, risk, kind, topn)
        plain = [j for _, j in sorted((-float(key[j]) + 0.0, j) for j in range(J))]
        assert expected_topn(mean, sd, rated[1][1], 1024, risk, False).tolist() == (plain + [-1] * 1024)[:1024]
        # and it is the order of the key's integer image with ~item behind it
        img = key_image(key)
        assert plain == sorted(range(J), key=lambda j: (-int(img[j]), j)), (name, sign, risk)
    assert seen >= {"all_equal", "two_values", "neighbours", "mirror", "wide", "ascending", "descending", "spread", "signed_zero"}


# ---- 3. every family has the property it exists for
def tie_straddles(key, topn):
    """places topn and topn + 1 of the order hold the same key"""
    k = np.sort(key_image(key))[::-1]
    return len(k) > topn and k[topn - 1] == k[topn]


def in_one_tie_run(key, a, b):
    return len(key) > b and key_image(key)[a] == key_image(key)[b]


@pytest.mark.parametrize("J", [4001, 70001])
def test_family_properties(J):
    fam = key_families(J, SEED)
    mean = {name: moments(sc)[0] for name, sc in fam.items()}
    for topn in TOPNS:
        for name in ("all_equal", "two_values_long", "signed_zero"):
            assert tie_straddles(mean[name], topn) and tie_straddles(-mean[name], topn), (name, topn)
        assert tie_straddles(-mean["two_values"], topn)  # the mirrored user's top is the long low run
    for topn in (1, 2):
        assert tie_straddles(mean["two_values"], topn)
    tv = fam["two_values"][0]
    for a, b in HIGH_RUNS:
        if J >= b:
            assert (tv[a:b] == tv.max()).all() and tv[a - 1] == tv[b] == tv.min()
    assert int((tv == tv.max()).sum()) == sum(b - a for a, b in HIGH_RUNS if J >= b)
    # tie runs across the bytes of ~item
    for name in ("all_equal", "two_values", "two_values_long"):
        assert in_one_tie_run(mean[name], 255, 256)
        if J > 65536:
            assert in_one_tie_run(mean[name], 65535, 65536), name
    # spread: items that share a mean but not a spread, so that risk reorders the ties
    m, v, sd = moments(fam["spread"])
    assert np.array_equal(v, sd * sd) and set(np.unique(sd)) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    for x in np.unique(m):
        assert len(np.unique(sd[m == x])) == 6
    assert tie_straddles(m - 1.0 * sd, 1024) and tie_straddles(m - 0.5 * sd, 1023)
    # neighbours: at least 256 distinct keys that share their top seven key bytes; denormals of both signs
    nb = fam["neighbours"][0]
    img = np.unique(key_image(nb))
    top7, cnt = np.unique(img >> np.uint64(8), return_counts=True)
    assert cnt.max() >= 256, cnt.max()
    tiny = np.finfo(np.float64).tiny
    assert ((nb > 0) & (nb < tiny)).sum() >= 300 and ((nb < 0) & (nb > -tiny)).sum() >= 300
    assert 1.0 in nb and np.nextafter(1.0, 2.0) in nb and np.nextafter(2.0, 0.0) in nb and np.nextafter(2.0, 3.0) in nb
    # both zeros
    a, b = ZERO_BLOCK
    assert np.all(nb[a:b] == 0.0) and np.array_equal(np.signbit(nb[a:b]), np.arange(a, b) % 2 == 1)
    sz = mean["signed_zero"]
    zero = sz == 0.0
    assert (zero & np.signbit(sz)).sum() > J // 4 and (zero & ~np.signbit(sz)).sum() > J // 4
    assert (sz == TINY).any() and (sz == -TINY).any()
    assert np.all(moments(fam["signed_zero"])[2] == 0.0)
    # mixed signs
    for name in ("wide", "mirror"):
        assert (fam[name][0] < 0).sum() >= J // 3 and (fam[name][0] > 0).sum() >= J // 3, name
    mg = np.abs(fam["mirror"][0])
    assert all(((fam["mirror"][0] == x).any() and (fam["mirror"][0] == -x).any()) for x in np.unique(mg))
    # wide: every byte of the key's image varies; squares overflow and underflow
    wi = key_image(fam["wide"][0])
    for byte in range(8):
        assert len(np.unique((wi >> np.uint64(8 * byte)) & np.uint64(255))) >= (128 if byte < 7 else 64), byte
    with np.errstate(all="ignore"):
        sq = fam["wide"][0] ** 2
    assert np.isinf(sq).sum() >= 8 and (sq == 0.0).sum() > J // 8
    wm, wv, wsd = moments(fam["wide"])
    assert np.isnan(wv).sum() >= 8 and np.all(wsd == 0.0)
    # ascending / descending: the winners in the row's last slots, or in thread 0's
    assert np.all(np.diff(fam["ascending"][0]) > 0) and np.all(np.diff(fam["descending"][0]) < 0)


def test_rated_kinds_hit_the_candidate_counts():
    for J in (1, 33, 1025, 4001):
        kinds = dict(rated_kinds(J, SEED))
        left = {J - len(r) for r in kinds.values()}
        want = {0, J} | {c for c in (1, 2, 3, 1022, 1023, 1024, 1025) if c < J}
        assert want <= left, (J, want - left)
        for r in kinds.values():
            assert len(np.unique(r)) == len(r) and (len(r) == 0 or r.max() < J)
        if J > 33:
            assert kinds["word_edge"].tolist() == [31, 32, 33, J - 1]


# ---- 4. moments on the exact construction
def test_moments_equal_rational_arithmetic():
    rng = np.random.default_rng(3)
    for S in (3, 4):
        I, J, K = 6, 9, 17
        U, V = rng.integers(-8, 9, (S, I, K)) / 4.0, rng.integers(-8, 9, (S, J, K)) / 4.0
        b0, bu, bv = rng.integers(-8, 9, S) / 4.0, rng.integers(-8, 9, (S, I)) / 4.0, rng.integers(-8, 9, (S, J)) / 4.0
        sc = np.stack([((b0[s] + bu[s])[:, None] + bv[s][None, :]) + U[s] @ V[s].T for s in range(S)])
        mean, v, sd = moments(sc)
        for i in range(I):
            for j in range(J):
                ex = [Fraction(b0[s]) + Fraction(bu[s, i]) + Fraction(bv[s, j])
                      + sum(Fraction(U[s, i, k]) * Fraction(V[s, j, k]) for k in range(K)) for s in range(S)]
                assert [Fraction(x) for x in sc[:, i, j]] == ex  # every score is exact
                s1, s2 = sum(ex), sum(x * x for x in ex)
                assert Fraction(float(s1)) == s1 and Fraction(float(s2)) == s2  # and so are the sums
                if S == 4:  # a power of two: mean and variance are the exact rationals
                    assert Fraction(mean[i, j]) == s1 / 4 and Fraction(v[i, j]) == s2 / 4 - (s1 / 4) ** 2
                    assert sd[i, j] == np.sqrt(v[i, j]) and v[i, j] >= 0
                else:  # each operation rounds once, in the kernel's order
                    m = float(s1) / S
                    assert mean[i, j] == m and abs(Fraction(m) - s1 / S) <= Fraction(abs(m)) * Fraction(1, 2 ** 53)
                    assert v[i, j] == float(s2) / S - m * m
    # S = 2 in small integers (the spread family): mean and variance are the exact rationals
    m0, d0 = rng.integers(-3, 4, 50).astype(float), rng.integers(0, 6, 50).astype(float)
    mean, v, sd = moments(np.stack([m0 + d0, m0 - d0]))
    for j in range(50):
        a, b = Fraction(m0[j] + d0[j]), Fraction(m0[j] - d0[j])
        em = (a + b) / 2
        ev = (a * a + b * b) / 2 - em * em
        assert Fraction(mean[j]) == em and Fraction(v[j]) == ev and Fraction(sd[j]) ** 2 == ev
    # one sample: the mean is the score, the variance exactly 0 (or NaN -> 0 where the square overflows)
    x = np.array([1.5, -2.25, 1e200, -0.0, TINY])
    mean, v, sd = moments(x[None])
    assert np.array_equal(mean, x) and not np.signbit(mean[3]) and np.all(sd == 0.0) and np.isnan(v[2])
