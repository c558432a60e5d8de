"""The two-attribute libFM learner's row forms (csrc/fmm.hip k_fmm_pass, k_fmm_chunk_draw,
k_fmm_item; host dispatch csrc/fmm.cpp run_bins, csrc/fmc.cpp fm_bin_rows / fm_cut_chunks) on the
rating set of tests/edge_rows.py: edge_rows.edge_set(17), the set tests/test_edge_rows_checker.py
validates -- 98,220 train and 1,732 test triples over 4,467 x 4,467 ids, two user rows and two item
rows of every length in edge_rows.LENGTHS (0 .. 4097), the empty rows present through num_users /
num_items and the test set.  No file is stored: that module is the data.

Which form a row of n cases runs on.  A row is binned by its length (fm_bin_rows, fmc.cpp:526-530:
n <= 256 bin 0, n <= SBMF_FMM_LONG bin 1, else bin 2; the bounds fm_long_bounds, fmc.cpp:520-524,
both 4096 by default) and a bin runs NT = 64 / 256 / 1024 threads per row (fm_bin_tpr, fmc.h:169).
A lane keeps its first MCF = 4 cases in registers (fmm.hip:106), so a row's first 4 NT cases are
"cached" from the sums to the residual update; the cases k >= 4 NT run in the two tail loops
(fmm.hip:133 the sums, fmm.hip:181 the update, which reloads them).  With one rank and
SBMF_FMM_CHUNK != 0 the rows of bin 2 are cut into ceil(n / chunk) near-equal chunks
(fm_cut_chunks, fmc.cpp:536-550; fmm.cpp:339-340): a sums launch over the chunks (xmode 1),
k_fmm_chunk_draw per row, and an update launch over the chunks (xmode 2, nothing cached: every
case reloaded, fmm.hip:110 and :168).

  one rank, default bounds (SBMF_FMM_LONG = SBMF_FMM_CHUNK = 4096)
    0..256      NT = 64, all cached (a row can hold at most 4 * 64 = 256 cases: no tail ever)
    257..1024   NT = 256, all cached
    1025..4096  NT = 256, 1 .. 3072 tail cases (1025: 1, 2047: 1023, 2048: 1024, 2049: 1025,
                4095: 3071, 4096: 3072)
    4097        2 chunks (2048 + 2049) on NT = 1024, k_fmm_chunk_draw
  chunk0 (SBMF_FMM_CHUNK=0)
    as default up to 4096; 4097 whole on NT = 1024 with 1 tail case
  long256-chunk64 (SBMF_FMM_LONG=256 SBMF_FMM_CHUNK=64)
    0..256 as default; 257 / 511, 512 / 513 / 1023, 1024 / 1025 / 2047, 2048 / 2049 / 4095, 4096 /
    4097 in 5 / 8 / 9 / 16 / 17 / 32 / 33 / 64 / 65 chunks of at most 64 on NT = 1024; bin 1 empty
  long256-chunk0 (SBMF_FMM_LONG=256 SBMF_FMM_CHUNK=0)
    0..256 as default; 257..4096 whole on NT = 1024, all cached; 4097: 1 tail case; bin 1 empty
  long8192 (SBMF_FMM_LONG=8192)
    as default up to 4096; 4097 on NT = 256 with a 3,073-case tail; bin 2 empty
  R > 1 ranks (users split into ranges by sbmf_partition_rows, fmm.cpp:280-293)
    user rows   whole on their rank by length as above, the scatter form (e_in -> e_out[perm], no
                e_io: fmm.cpp:94-98) and never in chunks (fmm.cpp:339): 4097 whole on NT = 1024
                with 1 tail case at default bounds
    item rows   every rank bins every item row by its local share (fmm.cpp:332): the sums launch
                (xmode 1) over that share, an all-gather, k_fmm_item (the R sums added in rank
                order), then the forwarding launch (xmode 2) that reloads every local case.  An
                edge item's cases come from random filler users, so its share differs from rank to
                rank and can sit in another bin on another rank; a 1-case item is a 0-case row of
                bin 0 on R - 1 ranks.
The general learner (SBMF_FMM_GENERAL=1, csrc/fmg.hip) bins and chunks the same rows by the same
host functions (fmg.cpp:86-106) and keeps the same MCF structure (fmg.hip:58-141).

expected_forms() restates the table; expected_pass_launches() derives from it the launches of one
pass over both sides as run_bins counts them (fmm.cpp:109-138: 3 per chunked bin, 1 per other
non-empty bin), which tests/test_gpu_fm_edge.py compares with timing().n_launch ("fm edge table
stale" when a bound moves).

Bars (tests/test_gpu_libfm.py's): train / test RMSE rtol 1e-9, U and V atol 1e-8, predict() atol
1e-9, biases and w0 1e-9, libFM's printed lines within half a unit of the sixth digit.
tests/test_fm_edge_checker.py shows on the CPU that a row computed without its last case is at
least 1,000 of these bars away, in its own v and in the train RMSE.
"""
import functools

import numpy as np

import edge_rows
from edge_rows import LENGTHS, SIDES

SET_SEED = 17
K, SEED, ITERS, INIT_STDEV = 8, 2, 3, 0.1
REGULAR = {"mcmc": (0.0, 0.0, 0.0), "als": (0.5, 1.0, 4.0)}
RTOL_RMSE, ATOL_FACTOR, ATOL_PRED, ATOL_BIAS = 1e-9, 1e-8, 1e-9, 1e-9
MCF = 4  # cases a lane keeps in registers (fmm.hip:106, fmg.hip)
BIN_NT = (64, 256, 1024)  # fm_bin_tpr
# the variants of tests/test_gpu_fm_edge.py: environment -> (SBMF_FMM_LONG, SBMF_FMM_CHUNK) as fm_long_bounds reads it
VARIANTS = {"default": {}, "chunk0": {"SBMF_FMM_CHUNK": "0"},
            "long256-chunk64": {"SBMF_FMM_LONG": "256", "SBMF_FMM_CHUNK": "64"},
            "long256-chunk0": {"SBMF_FMM_LONG": "256", "SBMF_FMM_CHUNK": "0"},
            "long8192": {"SBMF_FMM_LONG": "8192"}}


def bounds(env):
    """fm_long_bounds (fmc.cpp:520-524) on a variant's environment."""
    longb = max(256, int(env["SBMF_FMM_LONG"])) if "SBMF_FMM_LONG" in env else 4096
    chunk = max(0, int(env["SBMF_FMM_CHUNK"])) if "SBMF_FMM_CHUNK" in env else 4096
    return longb, chunk


def generate():
    """(train, test, (num_users, num_items)) of edge_rows.edge_set(SET_SEED)."""
    train, test, dims, _ = edge_rows.edge_set(SET_SEED)
    return train, test, dims


def rows_of(side):
    """{length: row ids} of the side's edge rows."""
    return edge_rows.edge_set(SET_SEED)[3][side]


def form(n, longb=4096, chunk=4096, ranks=1):
    """(bin, NT, chunks, tail cases) of a row whose n cases lie on one rank: chunks = 0 for a whole
    row; tail = the cases past the 4 NT a row's (or its longest chunk's) lanes keep in registers."""
    b = 0 if n <= 256 else 1 if n <= longb else 2
    nt = BIN_NT[b]
    chunks = -(-n // chunk) if (b == 2 and ranks == 1 and chunk) else 0
    longest = -(-n // chunks) if chunks else n  # fm_cut_chunks: pieces of floor / ceil (n / chunks)
    return b, nt, chunks, max(0, longest - MCF * nt)


def expected_forms(longb=4096, chunk=4096, ranks=1):
    """The table: {length: (bin, NT, chunks, tail cases)} for every edge length (with ranks > 1:
    the user rows; an item row's form follows its local share on each rank)."""
    return {n: form(n, longb, chunk, ranks) for n in LENGTHS}


def expected_pass_launches(longb=4096, chunk=4096):
    """Launches of one w or v pass over both sides on one rank (run_bins, fmm.cpp:109-138)."""
    total = 0
    for side in SIDES:
        bins = {}
        for n in edge_rows.degrees(SET_SEED, side):
            b, _, chunks, _ = form(int(n), longb, chunk)
            bins[b] = bins.get(b, False) or chunks > 0
        total += sum(3 if chunked else 1 for chunked in bins.values())
    return total


@functools.lru_cache(maxsize=None)
def oracle_run(method):
    """oracle.run_fmm on the set at the common settings (shared by the tests; read-only)."""
    import oracle
    train, test, dims = generate()
    o = oracle.run_fmm(train, test, K=K, iters=ITERS, seed=SEED, method=method, k0=1, k1=1, init_stdev=INIT_STDEV,
                       regular=REGULAR[method], num_users=dims[0])
    for a in o.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


def oracle_tables(o):
    """(U [I, K], V [J, K], bu, bv) of an oracle result, items past its attribute count read 0
    (FMChain::factors, fmc.cpp:499-518)."""
    _, _, (I, J) = generate()
    p = o["v"].shape[1]
    v = np.zeros((o["v"].shape[0], I + J))
    w = np.zeros(I + J)
    m = min(p, I + J)
    v[:, :m], w[:m] = o["v"][:, :m], o["w"][:m]
    return v[:, :I].T.copy(), v[:, I:].T.copy(), w[:I].copy(), w[I:].copy()


def by_length(side, err):
    """Print the largest error per edge length of the side and over its other rows (err: one
    value per row of the side, e.g. max |dU| over the factors); returns the lines."""
    err = np.asarray(err)
    rows = rows_of(side)
    edge = np.zeros(len(err), bool)
    lines = []
    for n in LENGTHS:
        edge[rows[n]] = True
        lines.append("%-6s %-7d %11.3e" % (side, n, err[rows[n]].max()))
    lines.append("%-6s %-7s %11.3e" % (side, "filler", err[~edge].max()))
    print("\n".join(["%-6s %-7s %11s" % ("side", "length", "max err")] + lines))
    return lines
