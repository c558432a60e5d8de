"""sbmf -- Python mirror of the reference's learner interface over the MI355X C ABI.

The reference's operator API for this path is libFM's ``fm_learn``
(src/libfm/src/fm_learn.h:38-308): ``init()``, ``learn(train, test)``,
``predict(data, out)``, ``evaluate(data)``, with the MCMC learner's knobs
``num_iter`` / ``num_eval_cases`` (fm_learn_mcmc.h:75-93) and the model's
``num_factor`` (fm_model.h:35-130).  ``FMLearnSBPMF`` keeps those names and
meanings; the work runs in ``libsbmf.so`` (HIP kernels for gfx950).  Errors
raise ``SBMFError`` (the reference throws ``std::string``).  There is no CPU
compute path: without a GPU, ``init()`` raises ``SBMFError`` (SBMF_E_DEVICE).

Runtime note: libsbmf binds ROCm's ``libamdhip64.so.7``.  PyTorch wheels ship
their own copy under the same soname; if torch is imported first, libsbmf
shares torch's runtime (fine).  If sbmf is imported first, create the learner
(``init()``) before the first ``torch.cuda`` call -- a second HSA runtime
initialised after the first one sees no device.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (F32, F64, METHOD_ALS, METHOD_LIBFM_MCMC, METHOD_MCMC, METHOD_VB, QUIRKS_BIAS2, QUIRKS_BIAS22, QUIRKS_FINAL, QUIRKS_NONE, QUIRKS_SBPMF2, RNG_PHILOX, RNG_REFERENCE, SBMF_E_ARG,
                   SBMF_E_COMM, SBMF_E_DEVICE, SBMF_E_IO, SBMF_E_NOMEM, SBMF_E_STATE, SBMF_OK)

__all__ = ["FMLearnSBPMF", "FMLearnVBOnline", "Data", "Cases", "Relation", "load_libfm_relation", "save_libfm_relation", "load_libfm_cases", "load_libfm_meta", "parse_regular", "fm_ranges", "SBMFError", "load_triples", "load_libfm", "load_libfm_binary", "save_libfm_binary", "libfm_binary_kind", "device_usage", "samples_file_info", "samples_hyper_file_info", "vb_posterior_file_info", "Communicator", "save_triples", "config_default",
           "RNG_REFERENCE", "RNG_PHILOX", "QUIRKS_FINAL", "QUIRKS_SBPMF2", "QUIRKS_NONE",
           "QUIRKS_BIAS2", "QUIRKS_BIAS22", "F64", "F32"]

lib = _lib.lib


class SBMFError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sbmf error %d: %s" % (code, msg))
        self.code = code


def _u32(a):
    """ids as uint32, refusing values the cast would wrap (negative or >= 2^32)."""
    a = np.asarray(a)
    if a.dtype != np.uint32 and a.size:
        if a.dtype.kind == "f" and not np.all(np.isfinite(a) & (a == np.floor(a))):
            raise ValueError("ids must be integers")
        if a.min() < 0 or a.max() > 0xffffffff:
            raise ValueError("ids must be in [0, 2^32 - 1]")
    return np.ascontiguousarray(a, dtype=np.uint32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Data:
    """Ratings triples (user, item, rating), 0-based ids; libFM's DataSubset role."""

    def __init__(self, user, item, rating):
        self.user, self.item, self.rating = _u32(user), _u32(item), _f64(rating)
        if not (len(self.user) == len(self.item) == len(self.rating)):
            raise ValueError("user/item/rating length mismatch")

    @property
    def num_cases(self):
        return len(self.rating)

    @property
    def target(self):
        return self.rating


class Cases:
    """A libFM data set with any number of features per case (sbmf_cases): a CSR by case.
    Case c holds the attributes attr[ptr[c]:ptr[c+1]] with the values x beside them and the
    target target[c]; x and target are libFM's DATA_FLOAT (float32).  num_attr defaults to the
    largest id + 1 (Data.h:220-222)."""

    def __init__(self, ptr, attr, x, target, num_attr=None):
        self.ptr = np.ascontiguousarray(ptr, dtype=np.uint64)
        self.attr = _u32(attr)
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.target = np.ascontiguousarray(target, dtype=np.float32)
        if len(self.ptr) != len(self.target) + 1 or len(self.attr) != len(self.x):
            raise ValueError("ptr / target or attr / x length mismatch")
        if int(self.ptr[0]) != 0 or int(self.ptr[-1]) != len(self.attr):
            raise ValueError("ptr must run from 0 to len(attr)")
        self.num_attr = int(num_attr) if num_attr is not None else (int(self.attr.max()) + 1 if len(self.attr) else 0)

    @property
    def num_cases(self):
        return len(self.target)

    @property
    def rating(self):  # the targets as float64 (what evaluate() compares against)
        return self.target.astype(np.float64)

    def _c(self):
        c = _lib.CasesC()
        c.n, c.nnz, c.num_attr = len(self.target), len(self.attr), self.num_attr
        c.ptr, c.attr = _ptr(self.ptr, C.c_uint64), _ptr(self.attr, C.c_uint32)
        c.x, c.target = _ptr(self.x, C.c_float), _ptr(self.target, C.c_float)
        return c


class Relation:
    """A block-structure relation (libFM's -relation; sbmf_add_relation): ``block`` is the block
    table as Cases (one row per block row, targets ignored), ``train_row`` / ``test_row`` the block
    row every train / test case joins, ``group`` the relation's own attribute groups ([block.num_attr],
    libFM's <stem>.groups) or None for one group."""

    def __init__(self, block, train_row, test_row=(), group=None):
        if not isinstance(block, Cases):
            raise ValueError("block must be Cases")
        self.block = block
        self.train_row, self.test_row = _u32(train_row).ravel(), _u32(test_row).ravel()
        self.group = None if group is None else _u32(group).ravel()
        if self.group is not None and len(self.group) != block.num_attr:
            raise ValueError("group must hold block.num_attr = %d ids; %d given" % (block.num_attr, len(self.group)))

    @property
    def num_groups(self):
        return int(self.group.max()) + 1 if self.group is not None and len(self.group) else 1


def load_libfm_relation(stem):
    """libFM's relation files <stem>.xt (or .x), <stem>.train, <stem>.test and the optional
    <stem>.groups as a Relation (sbmf_load_libfm_relation)."""
    c, G = _lib.CasesC(), C.c_uint32()
    tr, te, g = (C.POINTER(C.c_uint32)() for _ in range(3))
    ntr, nte = C.c_uint64(), C.c_uint64()
    rc = lib.sbmf_load_libfm_relation(str(stem).encode(), C.byref(c), C.byref(tr), C.byref(ntr), C.byref(te),
                                      C.byref(nte), C.byref(g), C.byref(G))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_loader_error().decode())
    try:
        arr = lambda p, m, t: np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0, t)
        n, nnz = int(c.n), int(c.nnz)
        block = Cases(arr(c.ptr, n + 1, np.uint64), arr(c.attr, nnz, np.uint32), arr(c.x, nnz, np.float32),
                      np.zeros(n, np.float32), num_attr=int(c.num_attr))
        return Relation(block, arr(tr, ntr.value, np.uint32), arr(te, nte.value, np.uint32),
                        arr(g, int(c.num_attr), np.uint32) if g else None)
    finally:
        lib.sbmf_free_relation(C.byref(c), C.byref(tr), C.byref(te), C.byref(g))


def save_libfm_relation(stem, relation, binary_maps=False):
    """Write <stem>.x (the block table, row-major: libFM's transpose tool makes the .xt its MCMC / ALS
    learner reads), <stem>.train / <stem>.test (text, or binary DVector<uint>) and, when the relation has
    groups, <stem>.groups."""
    c = relation.block._c()
    rc = lib.sbmf_save_libfm_block((str(stem) + ".x").encode(), C.byref(c))
    for ext, m in ((".train", relation.train_row), (".test", relation.test_row)):
        if rc == SBMF_OK:
            rc = lib.sbmf_save_libfm_row_map((str(stem) + ext).encode(), _ptr(m, C.c_uint32), len(m), 1 if binary_maps else 0)
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_loader_error().decode())
    if relation.group is not None:
        with open(str(stem) + ".groups", "w") as f:
            f.write("".join("%d\n" % x for x in relation.group))


def load_libfm_cases(path):
    """libFM text with any number of id:value features per line (Data.h:173-283):
    sbmf_load_libfm_cases.  Entries come back sorted by id within each case."""
    c = _lib.CasesC()
    rc = lib.sbmf_load_libfm_cases(str(path).encode(), C.byref(c))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_loader_error().decode())
    try:
        n, nnz = int(c.n), int(c.nnz)
        arr = lambda p, m, t: np.ctypeslib.as_array(p, shape=(m,)).copy() if m else np.zeros(0, t)
        return Cases(arr(c.ptr, n + 1, np.uint64), arr(c.attr, nnz, np.uint32), arr(c.x, nnz, np.float32),
                     arr(c.target, n, np.float32), num_attr=int(c.num_attr))
    finally:
        lib.sbmf_free_cases(C.byref(c))


def load_libfm_meta(path, num_attr):
    """A libFM -meta file (sbmf_load_libfm_meta): the group ids (uint32 [num_attr]) of the first
    num_attr whitespace-separated entries; fewer entries or a non-number raise SBMFError (SBMF_E_IO)."""
    out, G = np.zeros(int(num_attr), dtype=np.uint32), C.c_uint32()
    rc = lib.sbmf_load_libfm_meta(str(path).encode(), int(num_attr), _ptr(out, C.c_uint32), C.byref(G))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_loader_error().decode())
    return out


def parse_regular(regular, num_groups=1):
    """libFM's -regular (libfm.cpp:484-521) as (reg0, regw, regv, group_regw, group_regv): no value
    (all 0), one value for all, (r0, r1, r2), or with G = num_groups > 1 groups the 1 + 2G values
    (r0, w_lambda[0..G-1], v_lambda[0..G-1]); the group lists are None unless that form was given.
    For one group the two readings of three values coincide.  Any other count: ValueError."""
    r = [float(x) for x in (regular if np.ndim(regular) else [regular])]
    G = int(num_groups)
    if len(r) == 0:
        return 0.0, 0.0, 0.0, None, None
    if len(r) == 1:
        return r[0], r[0], r[0], None, None
    if len(r) == 3:
        return r[0], r[1], r[2], None, None
    if G > 1 and len(r) == 1 + 2 * G:
        return r[0], 0.0, 0.0, r[1:1 + G], r[1 + G:]
    raise ValueError("regular takes 0, 1 or 3 values, or 1 + 2G = %d with the %d attribute groups set; %d given"
                     % (1 + 2 * G, G, len(r)))


def fm_ranges(train, num_attr=None):
    """sbmf_fm_ranges: the bounds (uint32, [nranges + 1]) of the fewest contiguous id ranges of
    [0, num_attr) in which no training case holds two attributes."""
    p = train.num_attr if num_attr is None else int(num_attr)
    c, nr = train._c(), C.c_uint32()
    rc = lib.sbmf_fm_ranges(C.byref(c), p, None, 0, C.byref(nr))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    out = np.zeros(nr.value + 1, dtype=np.uint32)
    rc = lib.sbmf_fm_ranges(C.byref(c), p, _ptr(out, C.c_uint32), len(out), C.byref(nr))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    return out


def _from_ratings(r):
    n = int(r.n)
    if n == 0:
        return Data(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0))
    u = np.ctypeslib.as_array(r.user, shape=(n,)).copy()
    i = np.ctypeslib.as_array(r.item, shape=(n,)).copy()
    v = np.ctypeslib.as_array(r.rating, shape=(n,)).copy()
    return Data(u, i, v)


def load_triples(path):
    """SBPMF triple file (gibbs_sbpmf_final.cpp:43 acceptance rule)."""
    r = _lib.Ratings()
    rc = lib.sbmf_load_triples(str(path).encode(), C.byref(r))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_loader_error().decode())
    try:
        return _from_ratings(r)
    finally:
        lib.sbmf_free_ratings(C.byref(r))


def load_libfm_binary(stem, item_offset=0, transpose=False):
    """libFM binary <stem>.x/.y (or .data/.target), Data.h:113-160; one user and
    one item feature per row.  transpose=True reads the feature-major
    <stem>.xt/.y (or .datat/.target) that tools/transpose.cpp writes and
    bin/libFM -method mcmc|als loads (libfm.cpp:140-149)."""
    r = _lib.Ratings()
    fn = lib.sbmf_load_libfm_binary_t if transpose else lib.sbmf_load_libfm_binary
    rc = fn(str(stem).encode(), item_offset, C.byref(r))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_loader_error().decode())
    try:
        return _from_ratings(r)
    finally:
        lib.sbmf_free_ratings(C.byref(r))


def libfm_binary_kind(stem, has_x, has_xt):
    """Data::load's file choice (Data.h:112-117): 1 = .data/.datat/.target,
    2 = .x/.xt/.y, 0 = none (libFM text)."""
    rc = lib.sbmf_libfm_binary_kind(str(stem).encode(), int(has_x), int(has_xt))
    if rc < 0:
        raise SBMFError(rc, "has_x or has_xt must be set")
    return rc


def save_libfm_binary(stem, data, item_offset=0, num_cols=0, transpose=False):
    """Write <stem>.x / <stem>.y as tools/convert.cpp does for rating data
    (transpose=True: <stem>.xt / <stem>.y, convert then tools/transpose.cpp)."""
    u, i = _u32(data.user), _u32(data.item)  # refuses negative / >= 2^32 ids before the cast
    # the .x format holds feature ids (user, item_offset + item) as uint32 with num_cols = max + 1
    if len(u) and (int(u.max()) > 0xfffffffe or int(i.max()) + int(item_offset) > 0xfffffffe):
        raise ValueError("feature ids must stay below 2^32 - 1 in the libFM binary format")
    v = np.ascontiguousarray(data.rating, dtype=np.float64)
    r = _lib.Ratings()
    r.n = len(u)
    r.user = u.ctypes.data_as(C.POINTER(C.c_uint32))
    r.item = i.ctypes.data_as(C.POINTER(C.c_uint32))
    r.rating = v.ctypes.data_as(C.POINTER(C.c_double))
    fn = lib.sbmf_save_libfm_binary_t if transpose else lib.sbmf_save_libfm_binary
    rc = fn(str(stem).encode(), C.byref(r), item_offset, num_cols)
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_loader_error().decode())


def save_triples(path, data):
    """Write the SBPMF triple format (u\ti\tr per line) that load_triples reads back bit for bit."""
    u, i = _u32(data.user), _u32(data.item)
    v = np.ascontiguousarray(data.rating, dtype=np.float64)
    r = _lib.Ratings()
    r.n = len(u)
    r.user = u.ctypes.data_as(C.POINTER(C.c_uint32))
    r.item = i.ctypes.data_as(C.POINTER(C.c_uint32))
    r.rating = v.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.sbmf_save_triples(str(path).encode(), C.byref(r))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_loader_error().decode())


def load_libfm(path, item_offset=0):
    """libFM text with one user and one item feature per line (Data.h:192-217)."""
    r = _lib.Ratings()
    rc = lib.sbmf_load_libfm(str(path).encode(), item_offset, C.byref(r))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_loader_error().decode())
    try:
        return _from_ratings(r)
    finally:
        lib.sbmf_free_ratings(C.byref(r))


def libfm_users_first(train, test=None):
    """libFM's attribute split of a users-first file loaded with item_offset=0:
    num_user = max first feature id + 1 over train and test (libfm.cpp:219-221,
    263-265,375).  Returns (train, test, num_user) with the item ids rebased onto
    num_user -- pass num_user as set_data(..., num_users=num_user) so libFM's
    learners see the file's attribute ids, as the CLI does.  A file whose item ids
    do not all lie above every user id has no users-first reading: ValueError."""
    sets = [d for d in (train, test) if d is not None and d.num_cases]
    if not sets:
        return train, test, 0
    I = max(int(np.max(d.user)) for d in sets) + 1
    for d in sets:
        if int(np.min(d.item)) < I:
            raise ValueError("libFM input: item feature id %d <= the largest user feature id %d: not users first"
                             % (int(np.min(d.item)), I - 1))
    rebase = lambda d: None if d is None else Data(d.user, np.asarray(d.item, np.int64) - I, d.rating)
    return rebase(train), rebase(test), I


def _guest_csr(guests):
    """(n, ptr, items, ratings) of guests given as a list of (items, ratings) pairs or as a CSR
    tuple (ptr, items, ratings) of three 1-D numpy arrays."""
    if isinstance(guests, tuple) and len(guests) == 3 and all(isinstance(a, np.ndarray) and a.ndim == 1 for a in guests):
        ptr, items, ratings = _u32(guests[0]), _u32(guests[1]), _f64(guests[2])
    else:
        ptr = np.zeros(len(guests) + 1, dtype=np.int64)
        for g, (it, _) in enumerate(guests):
            ptr[g + 1] = ptr[g] + len(it)
        ptr = _u32(ptr)
        items = _u32(np.concatenate([np.asarray(it, dtype=np.int64).ravel() for it, _ in guests] + [np.zeros(0, np.int64)]))
        ratings = _f64(np.concatenate([np.asarray(r, dtype=np.float64).ravel() for _, r in guests] + [np.zeros(0)]))
        if len(items) != len(ratings):
            raise ValueError("a guest's items and ratings differ in length")
    n = max(len(ptr) - 1, 0)
    if n == 0:
        ptr = np.zeros(1, np.uint32)
    return n, ptr, items, ratings


def config_default():
    cfg = _lib.Config()
    lib.sbmf_config_default(C.byref(cfg))
    return cfg


class FMLearnSBPMF:
    """SBPMF Gibbs learner (fm_learn / fm_learn_mcmc shaped).

    Attributes mirror the reference: ``num_factor`` (K, -dim), ``num_iter``
    (-iter), ``seed``; plus the sampler's ``rng`` ("ref" | "philox"),
    ``quirks`` ("final" | "sbpmf2" | "none", or the biased sampler "bias2" |
    "bias22" = libFM ``-dim '1,1,K'``), ``precision`` ("f64" | "f32").
    ``rmse_trajectory`` collects the per-sweep running-mean test RMSE (the
    reference's ``rmse is`` lines / ``test_rmse_*`` file).
    """

    _QUIRKS = {"final": QUIRKS_FINAL, "sbpmf2": QUIRKS_SBPMF2, "none": QUIRKS_NONE, "bias2": QUIRKS_BIAS2,
               "bias22": QUIRKS_BIAS22}

    def __init__(self, num_factor=20, num_iter=100, seed=1, rng="ref", quirks="final", precision="f64", burnin=0,
                 device=0, init_stdev=None, recompute_every=1, eval_train=False,
                 stream_threshold=0, split_chunk=0, tune=0, method="mcmc", vb_batches=0, average="default",
                 order="sbpmf", k0=1, k1=1, regular=(0.0, 0.0, 0.0), task="r", **hyper):
        """method "mcmc" with order "sbpmf" (default): the SBPMF Gibbs sampler;
        method "mcmc" with order "libfm": libFM's own MCMC chain (f-outer, one
        hyperprior group, w0 / w with k0 / k1, -regular = ``regular``);
        "als": libFM's ALS (the same learner without sampling); "vb": online VB.
        With attribute groups (``set_groups``) ``regular`` may hold 1 + 2G values
        (r0, w_lambda per group, v_lambda per group), as libFM's -regular with -meta.
        task "c" (libFM's -task c; order "libfm" or method "als" only): binary classification with a
        probit model -- targets <= 0 are the negative class, ``history`` carries ``acc_train``,
        ``acc_avg``, ``acc_this`` and ``ll_this`` (the ``rmse_*`` are NaN), ``acc_trajectory`` is the
        running-mean test accuracy and ``predict()`` returns probabilities in [0, 1]."""
        self.cfg = config_default()
        if task not in ("r", "c"):
            raise ValueError("task must be r (regression) or c (classification)")
        self.cfg.task = _lib.TASK_CLASSIFICATION if task == "c" else _lib.TASK_REGRESSION
        if method not in ("mcmc", "vb", "vb_online", "als") or order not in ("sbpmf", "libfm"):
            raise ValueError("method must be mcmc, als or vb (order sbpmf or libfm)")
        if method in ("vb", "vb_online"):
            self.cfg.method = METHOD_VB
        elif method == "als":
            self.cfg.method = METHOD_ALS
        else:
            self.cfg.method = METHOD_LIBFM_MCMC if order == "libfm" else METHOD_MCMC
        self.cfg.libfm_dim = (1 if k0 else 0) | (2 if k1 else 0)
        self._regular, self._groups, self._relations = regular, None, []
        if np.ndim(regular) == 0 or len(regular) <= 3:  # the 1 + 2G form waits for set_groups
            self.cfg.reg0, self.cfg.regw, self.cfg.regv = parse_regular(regular)[:3]
        self.cfg.vb_batches = vb_batches
        self.cfg.num_factor = num_factor
        self.cfg.num_iter = num_iter
        self.cfg.burnin = burnin
        self.cfg.seed = seed
        self.cfg.rng_mode = RNG_PHILOX if rng == "philox" else RNG_REFERENCE
        self.cfg.quirks = self._QUIRKS[quirks]
        self.cfg.precision = F32 if precision == "f32" else F64
        self.cfg.device = device
        if init_stdev is not None:
            self.cfg.init_stdev = init_stdev
        self.cfg.recompute_every = recompute_every
        self.cfg.eval_train = 1 if eval_train else 0
        self.cfg.stream_threshold = stream_threshold
        self.cfg.split_chunk = split_chunk
        self.cfg.tune = tune
        # running-mean divisor: "default" (quirk set), "collected" (collected sweeps), "reference" (sweep + 1)
        self.cfg.average = {"default": 0, "collected": 1, "reference": 2}[average]
        for k, v in hyper.items():
            setattr(self.cfg, k, v)
        self.ctx = None
        self.history = []
        self._train = self._test = None

    # -- fm_learn::init (fm_learn.h:80)
    def init(self, comm=None):
        if self.ctx is not None:
            return
        ctx = C.c_void_p()
        rc = lib.sbmf_create(C.byref(self.cfg), C.byref(ctx))
        if rc != SBMF_OK:
            raise SBMFError(rc, lib.sbmf_last_global_error().decode())
        self.ctx = ctx
        if isinstance(comm, Communicator):  # a process-wide communicator, shared by learners in turn
            self._comm = comm  # keeps it alive as long as this learner
            self._check(lib.sbmf_comm_attach(self.ctx, comm.handle))
        elif comm is not None:  # (nranks, rank, 128-byte id): a communicator of this learner's own
            nranks, rank, uid = comm
            buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
            self._check(lib.sbmf_comm_init(self.ctx, nranks, rank, buf))

    def _check(self, rc):
        if rc != SBMF_OK:
            raise SBMFError(rc, lib.sbmf_last_error(self.ctx).decode())

    # what the score lists' and the sample store's wrappers share: ``fn`` is the library's entry
    # point, ``args`` its arguments between the context and the outputs
    def _topn(self, fn, n, topn, *args):
        """A top-N call for ``n`` rows: (ids int64 [n, topn] with -1 in empty slots, mean, stdev)."""
        if not 0 <= int(topn) <= 0xffffffff:
            raise ValueError("topn must be a non-negative 32-bit count")
        t = int(topn)
        ids = np.full((max(n, 1), max(t, 1)), 0xffffffff, dtype=np.uint32)
        mean, sd = np.full(ids.shape, np.nan), np.full(ids.shape, np.nan)
        self._check(fn(self.ctx, *args, _ptr(ids, C.c_uint32), _ptr(mean, C.c_double), _ptr(sd, C.c_double)))
        out = ids[:n, :t].astype(np.int64)
        out[out == 0xffffffff] = -1
        return out, mean[:n, :t], sd[:n, :t]

    def _scores(self, fn, width, *args):
        """A (mean, stdev) call with ``width`` values each."""
        mean, sd = np.zeros(max(width, 1)), np.zeros(max(width, 1))
        self._check(fn(self.ctx, *args, _ptr(mean, C.c_double), _ptr(sd, C.c_double)))
        return mean[:width], sd[:width]

    def _ms(self, fn, *names):
        """A timing call: {name: device ms}."""
        ms = [C.c_double() for _ in names]
        self._check(fn(self.ctx, *[C.byref(m) for m in ms]))
        return {k: m.value for k, m in zip(names, ms)}

    def set_groups(self, group):
        """libFM's -meta: group[a] is the attribute group of attribute a, for every a < num_attribute
        (the largest attribute id over train and test + 2; for triples user u is attribute u and
        item i attribute num_users + i).  libFM's MCMC / ALS learners then draw w_mu, w_lambda,
        v_mu, v_lambda per group.  Call before set_data; an empty list drops the groups.  Triples
        given groups run through the general learner (fm_info() / fm() then work)."""
        g = _u32(group).ravel()
        self._groups = g if len(g) else None
        if self.ctx is not None:
            self._send_groups()

    def add_relation(self, relation):
        """libFM's -relation: register a Relation, in -relation order, before set_data.  Its
        attributes follow the main table's ids and its groups the main table's groups; fm(),
        fm_info() and fm_groups() then speak of the joined spaces (fm_relation_info() has the
        offsets) and ``regular`` in its per-group form takes 1 + 2G values over all groups."""
        if not isinstance(relation, Relation):
            raise ValueError("add_relation takes a Relation")
        if self._train is not None:
            raise SBMFError(SBMF_E_STATE, "add_relation: the data is already set")
        self._relations.append(relation)

    def _send_relations(self):
        for r in self._relations:
            c = r.block._c()
            g = r.group
            self._check(lib.sbmf_add_relation(self.ctx, C.byref(c), _ptr(r.train_row, C.c_uint32), len(r.train_row),
                                              _ptr(r.test_row, C.c_uint32), len(r.test_row),
                                              _ptr(g, C.c_uint32) if g is not None else None,
                                              r.num_groups if g is not None else 0))

    def fm_relation_info(self):
        """sbmf_fm_relation_info: one dict per relation -- attr_offset, num_attr, block_rows, nranges,
        group_offset, num_groups."""
        n = C.c_uint32()
        self._check(lib.sbmf_fm_relation_info(self.ctx, C.byref(n), 0, None, None, None, None, None, None))
        a = [np.zeros(max(n.value, 1), np.uint32) for _ in range(6)]
        self._check(lib.sbmf_fm_relation_info(self.ctx, C.byref(n), n.value, *[_ptr(x, C.c_uint32) for x in a]))
        keys = ("attr_offset", "num_attr", "block_rows", "nranges", "group_offset", "num_groups")
        return [{k: int(x[r]) for k, x in zip(keys, a)} for r in range(n.value)]

    def _send_groups(self):
        g = self._groups
        G = (int(g.max()) + 1 if g is not None else 1) + sum(r.num_groups for r in self._relations)
        r0, rw, rv, gw, gv = parse_regular(self._regular, G)
        if self.ctx is None:  # the context is created with reg0 (the per-group values go to it below)
            self.cfg.reg0, self.cfg.regw, self.cfg.regv = r0, rw, rv
            self.init()
        self._check(lib.sbmf_set_attr_groups(self.ctx, len(g) if g is not None else 0,
                                             _ptr(g, C.c_uint32) if g is not None else None))
        if gw is not None:
            gw, gv = _f64(gw), _f64(gv)
            self._check(lib.sbmf_set_group_regular(self.ctx, G, _ptr(gw, C.c_double), _ptr(gv, C.c_double)))

    def fm_groups(self):
        """sbmf_get_fm_groups: {"G", "cnt" [G], "w_lambda" [G], "w_mu" [G], "v_lambda" [G, K], "v_mu" [G, K]}."""
        G, K = C.c_uint32(), self.cfg.num_factor
        self._check(lib.sbmf_get_fm_groups(self.ctx, C.byref(G), None, None, None, None, None))
        n = G.value
        cnt, wl, wm = np.zeros(n, np.uint32), np.zeros(n), np.zeros(n)
        vl, vm = np.zeros((n, K)), np.zeros((n, K))
        self._check(lib.sbmf_get_fm_groups(self.ctx, C.byref(G), _ptr(cnt, C.c_uint32), _ptr(wl, C.c_double),
                                           _ptr(wm, C.c_double), _ptr(vl, C.c_double), _ptr(vm, C.c_double)))
        return {"G": n, "cnt": cnt, "w_lambda": wl, "w_mu": wm, "v_lambda": vl, "v_mu": vm}

    def set_data(self, train, test=None, num_users=0, num_items=0):
        grouped = self._groups is not None or not (np.ndim(self._regular) == 0 or len(self._regular) <= 3)
        # relations are checked against the data, and the per-group -regular counts their groups:
        # with relations the groups go after them, else before the data as always
        if grouped and not self._relations:
            self._send_groups()
        if self._relations and self.ctx is None:
            G = (int(self._groups.max()) + 1 if self._groups is not None else 1) + sum(r.num_groups for r in self._relations)
            self.cfg.reg0, self.cfg.regw, self.cfg.regv = parse_regular(self._regular, G)[:3]
        self.init()
        self._train, self._test = train, test
        if isinstance(train, Cases):  # libFM order / ALS: cases with any number of features
            if test is not None and not isinstance(test, Cases):
                raise ValueError("train and test must both be Cases")
            c = train._c()
            self._check(lib.sbmf_set_train_cases(self.ctx, C.byref(c)))
            if test is not None:
                c = test._c()
                self._check(lib.sbmf_set_test_cases(self.ctx, C.byref(c)))
        else:
            self._check(lib.sbmf_set_train(self.ctx, train.num_cases, _ptr(train.user, C.c_uint32),
                                           _ptr(train.item, C.c_uint32), _ptr(train.rating, C.c_double)))
            if test is not None:
                self._check(lib.sbmf_set_test(self.ctx, test.num_cases, _ptr(test.user, C.c_uint32),
                                              _ptr(test.item, C.c_uint32), _ptr(test.rating, C.c_double)))
            if num_users or num_items:
                self._check(lib.sbmf_set_dims(self.ctx, num_users, num_items))
        if self._relations:
            self._send_relations()
            self._send_groups()
        self._check(lib.sbmf_prepare(self.ctx))

    # -- fm_learn::learn(train, test) (fm_learn.h:150; fm_learn_mcmc.h:1154)
    def learn(self, train=None, test=None, sweeps=None, callback=None):
        if train is not None:
            self.set_data(train, test)
        n = self.cfg.num_iter + self.cfg.burnin if sweeps is None else sweeps

        def _cb(info_p, _user):
            info = info_p.contents
            rec = {f: getattr(info, f) for f, _ in _lib.SweepInfo._fields_}
            self.history.append(rec)
            return 1 if (callback is not None and callback(rec)) else 0

        cb = _lib.SWEEP_CB(_cb)
        self._check(lib.sbmf_run(self.ctx, n, cb, None))
        return self.history

    @property
    def rmse_trajectory(self):
        return np.array([h["rmse_avg"] for h in self.history])

    @property
    def acc_trajectory(self):
        """task "c": the per-sweep test accuracy of the running-mean probability (libFM's "Test=")."""
        return np.array([h["acc_avg"] for h in self.history])

    # -- fm_learn::predict (fm_learn.h:191): averaged clamped predictions of the test set (task "c":
    # the probabilities of the positive class, clipped to [0, 1])
    def predict(self):
        out = np.zeros(self._test.num_cases if self._test is not None else 0)
        self._check(lib.sbmf_predict(self.ctx, _ptr(out, C.c_double)))
        return out

    # -- fm_learn::evaluate (fm_learn.h:135): RMSE of the averaged prediction
    def evaluate(self):
        p = self.predict()
        return float(np.sqrt(np.mean((p - self._test.rating) ** 2)))

    def dims(self):
        nu, ni = C.c_uint32(), C.c_uint32()
        ntr, nte = C.c_uint64(), C.c_uint64()
        self._check(lib.sbmf_get_dims(self.ctx, C.byref(nu), C.byref(ni), C.byref(ntr), C.byref(nte)))
        return nu.value, ni.value, ntr.value, nte.value

    def factors(self):
        nu, ni, _, _ = self.dims()
        K = self.cfg.num_factor
        U = np.zeros((nu, K))
        V = np.zeros((ni, K))
        self._check(lib.sbmf_get_factors(self.ctx, _ptr(U, C.c_double), _ptr(V, C.c_double)))
        return U, V

    def set_factors(self, U, V):
        U, V = _f64(U), _f64(V)
        self._check(lib.sbmf_set_factors(self.ctx, _ptr(U, C.c_double), _ptr(V, C.c_double)))

    def hyper(self):
        K = self.cfg.num_factor
        h = np.zeros(4 * K)
        tau = C.c_double()
        self._check(lib.sbmf_get_hyper(self.ctx, _ptr(h, C.c_double), C.byref(tau)))
        return {"sigma_u": h[:K], "mu_u": h[K:2 * K], "sigma_v": h[2 * K:3 * K], "mu_v": h[3 * K:], "tau": tau.value}

    def biases(self):
        """Biased sampler: (b_i [users], b_j [items], b_0)."""
        nu, ni, _, _ = self.dims()
        bu, bv, b0 = np.zeros(nu), np.zeros(ni), C.c_double()
        self._check(lib.sbmf_get_biases(self.ctx, _ptr(bu, C.c_double), _ptr(bv, C.c_double), C.byref(b0)))
        return bu, bv, b0.value

    def fm_info(self):
        """The general libFM learner (set_data with Cases, or SBMF_FMM_GENERAL=1): libFM's
        num_attribute, the ranges of mutually exclusive attributes, and the kernel launches of
        the last iteration."""
        a, r, l = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(lib.sbmf_fm_info(self.ctx, C.byref(a), C.byref(r), C.byref(l)))
        return {"num_attr": a.value, "nranges": r.value, "launches_per_iter": l.value}

    def fm(self):
        """The general libFM learner's model (w0, w [num_attr], v [K, num_attr])."""
        p, K = self.fm_info()["num_attr"], self.cfg.num_factor
        w0, w, v = C.c_double(), np.zeros(p), np.zeros((K, p))
        self._check(lib.sbmf_get_fm(self.ctx, C.byref(w0), _ptr(w, C.c_double), _ptr(v, C.c_double)))
        return w0.value, w, v

    def timing(self):
        t = _lib.Timing()
        self._check(lib.sbmf_get_timing(self.ctx, C.byref(t)))
        return t

    # -- posterior top-N for a watch list of users (include/sbmf.h; not a reference interface)
    def watch(self, users, clamp=False):
        """Track the score of every item for these users (ids may repeat) from the next
        sweep on: sbmf_watch_users.  ``clamp``: clamp each sweep's score like the test
        prediction.  An empty list drops the watch and frees its device buffers."""
        users = _u32(users).ravel()
        self._check(lib.sbmf_watch_users(self.ctx, len(users), _ptr(users, C.c_uint32), 1 if clamp else 0))
        self._n_watch = len(users)

    def watch_scores(self, w):
        """(mean, stdev) of watched user ``w`` (index into the list) over the sweeps
        collected since ``watch``, one value per item."""
        return self._scores(lib.sbmf_watch_scores, self.dims()[1], int(w))

    def recommend(self, topn=10, exclude_rated=True, risk=0.0):
        """Per watched user the ``topn`` items with the largest mean - risk * stdev (ties by
        ascending item id), without the items the user rated in training unless
        ``exclude_rated`` is False.  Returns (items int64 [n, topn] with -1 in empty
        slots, mean, stdev); empty slots hold NaN."""
        return self._topn(lib.sbmf_recommend, getattr(self, "_n_watch", 0), topn, int(topn), 0 if exclude_rated else 1,
                          float(risk))

    def watch_timing(self):
        """Device ms of the last sweep's scoring launch and of the last selection."""
        return self._ms(lib.sbmf_watch_timing, "ms_score", "ms_select")

    # -- posterior sample store: thinned samples of the chain kept on the device, scored after the run
    def keep_samples(self, every=1, cap=64):
        """Keep every ``every``-th collected sweep from now on in a ring of ``cap`` samples
        (sbmf_keep_samples); ``cap`` 0 drops the store and frees its device buffers."""
        self._check(lib.sbmf_keep_samples(self.ctx, int(every), int(cap)))

    def samples_info(self):
        """{"count", "cap", "every", "bytes"} of the store."""
        c, k, e, b = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._check(lib.sbmf_samples_info(self.ctx, C.byref(c), C.byref(k), C.byref(e), C.byref(b)))
        return {"count": c.value, "cap": k.value, "every": e.value, "bytes": b.value}

    def sample(self, s):
        """Stored sample ``s`` (0 the oldest): {"sweep", "U" [users, K], "V" [items, K], "bu", "bv", "b0"}."""
        nu, ni, _, _ = self.dims()
        K = self.cfg.num_factor
        U, V, bu, bv = np.zeros((nu, K)), np.zeros((ni, K)), np.zeros(nu), np.zeros(ni)
        sw, b0 = C.c_uint32(), C.c_double()
        self._check(lib.sbmf_get_sample(self.ctx, int(s), C.byref(sw), _ptr(U, C.c_double), _ptr(V, C.c_double),
                                        _ptr(bu, C.c_double), _ptr(bv, C.c_double), C.byref(b0)))
        return {"sweep": sw.value, "U": U, "V": V, "bu": bu, "bv": bv, "b0": b0.value}

    def samples_scores(self, user, clamp=False):
        """(mean, stdev) of ``user``'s score of every item over the stored samples."""
        return self._scores(lib.sbmf_samples_scores, self.dims()[1], int(user), 2 if clamp else 0)

    def samples_recommend(self, users, topn=10, exclude_rated=True, risk=0.0, clamp=False):
        """``recommend`` for any users, named now, from the stored samples: (items int64
        [n, topn] with -1 in empty slots, mean, stdev)."""
        users = _u32(users).ravel()
        flags = (0 if exclude_rated else 1) | (2 if clamp else 0)
        return self._topn(lib.sbmf_samples_recommend, len(users), topn, len(users), _ptr(users, C.c_uint32), int(topn),
                          flags, float(risk))

    def samples_predict(self, users, items, clamp=False):
        """(mean, stdev) of the pairs (users[p], items[p]) over the stored samples."""
        users, items = _u32(users).ravel(), _u32(items).ravel()
        if len(users) != len(items):
            raise ValueError("users and items must have the same length")
        return self._scores(lib.sbmf_samples_predict, len(users), len(users), _ptr(users, C.c_uint32),
                            _ptr(items, C.c_uint32), 2 if clamp else 0)

    def samples_timing(self):
        """Device ms of the last copy into the store, the last scoring launch and the last selection."""
        return self._ms(lib.sbmf_samples_timing, "ms_copy", "ms_score", "ms_select")

    def save_samples(self, path):
        self._check(lib.sbmf_save_samples(self.ctx, str(path).encode()))

    def load_samples(self, path):
        """Replace the store by a sample file's (a prepared learner of the same dims, K,
        precision and quirk-set bias-ness; no sweep needed)."""
        self._check(lib.sbmf_load_samples(self.ctx, str(path).encode()))

    # -- guests folded into the stored samples after the run (no sweep; also from files)
    def sample_hyper(self, s):
        """The hyperparameters of stored sample ``s`` (0 the oldest), as ``hyper()`` returns the chain's."""
        K = self.cfg.num_factor
        h = np.zeros(4 * K)
        tau = C.c_double()
        self._check(lib.sbmf_get_sample_hyper(self.ctx, int(s), _ptr(h, C.c_double), C.byref(tau)))
        return {"sigma_u": h[:K], "mu_u": h[K:2 * K], "sigma_v": h[2 * K:3 * K], "mu_v": h[3 * K:], "tau": tau.value}

    def save_samples_hyper(self, path):
        """The samples' hyperparameters to the companion file of ``save_samples``' file."""
        self._check(lib.sbmf_save_samples_hyper(self.ctx, str(path).encode()))

    def load_samples_hyper(self, path):
        """The companion file's hyperparameters for the samples ``load_samples`` loaded."""
        self._check(lib.sbmf_load_samples_hyper(self.ctx, str(path).encode()))

    def samples_foldin_recommend(self, guests, topn=10, exclude_rated=True, risk=0.0, clamp=False, scans=1):
        """``foldin_recommend`` from the stored samples for guests named now (the form ``foldin``
        takes): (items int64 [n, topn] with -1 in empty slots, mean, stdev).  ``scans``: coordinate
        scans per sample (sbmf_samples_foldin_recommend)."""
        n, ptr, items, ratings = _guest_csr(guests)
        flags = (0 if exclude_rated else 1) | (2 if clamp else 0)
        return self._topn(lib.sbmf_samples_foldin_recommend, n, topn, n, _ptr(ptr, C.c_uint32), _ptr(items, C.c_uint32),
                          _ptr(ratings, C.c_double), int(scans), int(topn), flags, float(risk))

    def samples_foldin_rows(self, guests, scans=1):
        """The guests' factor rows at every stored sample, [count, n, K], oldest sample first."""
        n, ptr, items, ratings = _guest_csr(guests)
        count = self.samples_info()["count"]
        rows = np.zeros((max(count, 1), max(n, 1), self.cfg.num_factor))  # (n = 0: nothing is written)
        self._check(lib.sbmf_samples_foldin_rows(self.ctx, n, _ptr(ptr, C.c_uint32), _ptr(items, C.c_uint32),
                                                 _ptr(ratings, C.c_double), int(scans), _ptr(rows, C.c_double)))
        return rows[:count, :n]

    def samples_foldin_scores(self, items, ratings, clamp=False, scans=1):
        """(mean, stdev) of one guest's score of every item over the stored samples (the guest is
        drawn as guest 0 of a list)."""
        items, ratings = _u32(np.asarray(items, dtype=np.int64).ravel()), _f64(np.asarray(ratings, dtype=np.float64).ravel())
        if len(items) != len(ratings):
            raise ValueError("items and ratings differ in length")
        return self._scores(lib.sbmf_samples_foldin_scores, self.dims()[1], len(items), _ptr(items, C.c_uint32),
                            _ptr(ratings, C.c_double), int(scans), 2 if clamp else 0)

    def samples_foldin_timing(self):
        """Device ms of the last guest call's draw, scoring launch and selection (its last slice)."""
        return self._ms(lib.sbmf_samples_foldin_timing, "ms_draw", "ms_score", "ms_select")

    # -- posterior top-N for guests: users outside the training set, given by their ratings
    def foldin(self, guests, clamp=False):
        """Register a fold-in list (sbmf_foldin_users): ``guests`` is a list of
        (items, ratings) pairs, one per guest (both may be empty), or a CSR as a tuple
        (ptr, items, ratings) of three 1-D numpy arrays.  From the next sweep on every guest's
        factor row is drawn beside the chain and its scores accumulated on collected
        sweeps.  An empty list drops the fold-in list and frees its device buffers."""
        n, ptr, items, ratings = _guest_csr(guests)
        self._check(lib.sbmf_foldin_users(self.ctx, n, _ptr(ptr, C.c_uint32), _ptr(items, C.c_uint32),
                                          _ptr(ratings, C.c_double), 1 if clamp else 0))
        self._n_guests = n

    def foldin_factors(self):
        """The current sample's guest rows [n, K] (the last sweep's draw)."""
        rows = np.zeros((max(getattr(self, "_n_guests", 0), 1), self.cfg.num_factor))
        self._check(lib.sbmf_foldin_factors(self.ctx, _ptr(rows, C.c_double)))
        return rows[:getattr(self, "_n_guests", 0)]

    def foldin_scores(self, g):
        """(mean, stdev) of guest ``g`` over the sweeps collected since ``foldin``, one value per item."""
        return self._scores(lib.sbmf_foldin_scores, self.dims()[1], int(g))

    def foldin_recommend(self, topn=10, exclude_rated=True, risk=0.0):
        """``recommend`` for the guests; "rated" means the guest's own items."""
        return self._topn(lib.sbmf_foldin_recommend, getattr(self, "_n_guests", 0), topn, int(topn),
                          0 if exclude_rated else 1, float(risk))

    def foldin_timing(self):
        """Device ms of the last sweep's draw and scoring launch and of the last selection."""
        return self._ms(lib.sbmf_foldin_timing, "ms_draw", "ms_score", "ms_select")

    # -- posterior top-N of query cases over a relation's block rows (libFM's MCMC / ALS learner)
    def fm_queries(self, relation, cases, rows=None, exclude=None, clamp=False):
        """Register a query list (sbmf_fm_query_cases): ``relation`` is the index of the relation
        whose block rows are ranked, ``cases`` the queries' main-table features as Cases (targets
        ignored), ``rows`` one sequence of block-row indices per relation (the candidates' entry
        may be None; ``rows`` itself may be None with one relation), ``exclude`` per query the
        block rows left out of its top-N -- a list of sequences, or a CSR (ptr, rows) of two 1-D
        numpy arrays.  From the next iteration on every query's score against every block row is
        accumulated; ``clamp`` clamps each iteration's score like the test prediction.  Cases
        without a case drop the list and free its device buffers."""
        if not isinstance(cases, Cases):
            raise ValueError("fm_queries takes Cases")
        n = cases.num_cases
        nrel = len(self._relations)
        keep = [None] * nrel  # the arrays the pointer table points into
        arr = (_lib._P_U32 * max(nrel, 1))()
        for r in range(nrel):
            if rows is not None and r < len(rows) and rows[r] is not None:
                keep[r] = _u32(rows[r]).ravel()
                if len(keep[r]) != n:
                    raise ValueError("rows[%d] holds %d block rows; %d queries" % (r, len(keep[r]), n))
                arr[r] = _ptr(keep[r], C.c_uint32)
        eptr = erows = None
        if exclude is not None:
            if isinstance(exclude, tuple) and len(exclude) == 2 and all(isinstance(a, np.ndarray) and a.ndim == 1 for a in exclude):
                eptr, erows = _u32(exclude[0]), _u32(exclude[1])
            else:
                if len(exclude) != n:
                    raise ValueError("exclude holds %d lists; %d queries" % (len(exclude), n))
                eptr = _u32(np.concatenate([[0], np.cumsum([len(e) for e in exclude])]))
                erows = _u32(np.concatenate([np.asarray(e, dtype=np.int64).ravel() for e in exclude] + [np.zeros(0, np.int64)]))
            if len(eptr) != n + 1:
                raise ValueError("the exclusion ptr holds %d values; %d queries" % (len(eptr), n))
            if len(erows) == 0:
                erows = np.zeros(1, np.uint32)
        c = cases._c()
        self._check(lib.sbmf_fm_query_cases(self.ctx, int(relation), C.byref(c), arr if nrel else None,
                                            _ptr(eptr, C.c_uint32) if eptr is not None else None,
                                            _ptr(erows, C.c_uint32) if erows is not None else None, 1 if clamp else 0))
        self._n_queries = n
        self._query_rows = self.fm_relation_info()[int(relation)]["block_rows"] if n else 0

    def fm_query_scores(self, q):
        """(mean, stdev) of query ``q`` over the iterations accumulated since ``fm_queries`` (ALS: the
        latest iteration, stdev 0), one value per block row of the candidates' relation."""
        return self._scores(lib.sbmf_fm_query_scores, getattr(self, "_query_rows", 0), int(q))

    def fm_query_recommend(self, topn=10, risk=0.0, keep_excluded=False):
        """Per query the ``topn`` block rows with the largest mean - risk * stdev (ties by ascending
        row), without the query's excluded rows unless ``keep_excluded``.  Returns (rows int64
        [n, topn] with -1 in empty slots, mean, stdev); empty slots hold NaN."""
        return self._topn(lib.sbmf_fm_query_recommend, getattr(self, "_n_queries", 0), topn, int(topn),
                          1 if keep_excluded else 0, float(risk))

    def fm_query_timing(self):
        """Device ms of the last iteration's query terms and operand copy, of its scoring launch,
        and of the last selection."""
        return self._ms(lib.sbmf_fm_query_timing, "ms_terms", "ms_score", "ms_select")

    # -- online VB: the posterior, closed-form top-N for users and guests, the model file
    def vb_posterior(self):
        """The online VB learner's posterior means and variances (sbmf_vb_get_posterior): a dict
        with U_mean, U_var [users, K], V_mean, V_var [items, K], bu_mean, bu_var [users], bv_mean,
        bv_var [items], b0 = (mean, variance), alpha, sigma_0, sigma_w and sigma_v [K]."""
        nu, ni, _, _ = self.dims()
        K = self.cfg.num_factor
        shapes = (("U_mean", (nu, K)), ("U_var", (nu, K)), ("V_mean", (ni, K)), ("V_var", (ni, K)), ("bu_mean", (nu,)),
                  ("bu_var", (nu,)), ("bv_mean", (ni,)), ("bv_var", (ni,)))
        out = {k: np.zeros(s) for k, s in shapes}
        b0, hy = np.zeros(2), np.zeros(K + 3)
        self._check(lib.sbmf_vb_get_posterior(self.ctx, *[_ptr(out[k], C.c_double) for k, _ in shapes],
                                              _ptr(b0, C.c_double), _ptr(hy, C.c_double)))
        out.update(b0=(b0[0], b0[1]), alpha=hy[0], sigma_0=hy[1], sigma_w=hy[2], sigma_v=hy[3:].copy())
        return out

    def vb_scores(self, user):
        """(mean, stdev) of ``user``'s score of every item under the VB posterior (closed form)."""
        return self._scores(lib.sbmf_vb_scores, self.dims()[1], int(user))

    def vb_recommend(self, users, topn=10, exclude_rated=True, risk=0.0):
        """Per named user the ``topn`` items with the largest mean - risk * stdev under the VB
        posterior: (items int64 [n, topn] with -1 in empty slots, mean, stdev)."""
        users = _u32(users).ravel()
        return self._topn(lib.sbmf_vb_recommend, len(users), topn, len(users), _ptr(users, C.c_uint32), int(topn),
                          0 if exclude_rated else 1, float(risk))

    def vb_predict(self, users, items):
        """(mean, stdev) of the pairs (users[p], items[p]) under the VB posterior; no clamp."""
        users, items = _u32(users).ravel(), _u32(items).ravel()
        if len(users) != len(items):
            raise ValueError("users and items must have the same length")
        return self._scores(lib.sbmf_vb_predict, len(users), len(users), _ptr(users, C.c_uint32), _ptr(items, C.c_uint32))

    def vb_foldin_rows(self, guests, scans=1):
        """The guests' posterior (the form ``foldin`` takes), items held fixed, after ``scans``
        coordinate scans: (row_mean [n, K], row_var [n, K], b_mean [n], b_var [n])."""
        n, ptr, items, ratings = _guest_csr(guests)
        K = self.cfg.num_factor
        rm, rv, bm, bv = np.zeros((max(n, 1), K)), np.zeros((max(n, 1), K)), np.zeros(max(n, 1)), np.zeros(max(n, 1))
        self._check(lib.sbmf_vb_foldin_rows(self.ctx, n, _ptr(ptr, C.c_uint32), _ptr(items, C.c_uint32),
                                            _ptr(ratings, C.c_double), int(scans), _ptr(rm, C.c_double),
                                            _ptr(rv, C.c_double), _ptr(bm, C.c_double), _ptr(bv, C.c_double)))
        return rm[:n], rv[:n], bm[:n], bv[:n]

    def vb_foldin_scores(self, items, ratings, scans=1):
        """(mean, stdev) of one guest's score of every item under its VB posterior."""
        items, ratings = _u32(np.asarray(items, dtype=np.int64).ravel()), _f64(np.asarray(ratings, dtype=np.float64).ravel())
        if len(items) != len(ratings):
            raise ValueError("items and ratings differ in length")
        return self._scores(lib.sbmf_vb_foldin_scores, self.dims()[1], len(items), _ptr(items, C.c_uint32),
                            _ptr(ratings, C.c_double), int(scans))

    def vb_foldin_recommend(self, guests, topn=10, exclude_rated=True, risk=0.0, scans=1):
        """``vb_recommend`` for guests named now; "rated" means the guest's own items."""
        n, ptr, items, ratings = _guest_csr(guests)
        return self._topn(lib.sbmf_vb_foldin_recommend, n, topn, n, _ptr(ptr, C.c_uint32), _ptr(items, C.c_uint32),
                          _ptr(ratings, C.c_double), int(scans), int(topn), 0 if exclude_rated else 1, float(risk))

    def save_vb_posterior(self, path):
        self._check(lib.sbmf_vb_save_posterior(self.ctx, str(path).encode()))

    def load_vb_posterior(self, path):
        """Replace the posterior by a file's (a prepared VB learner of the same dims and K; no
        epoch needed).  ``learn`` is refused afterwards: the file holds no training state."""
        self._check(lib.sbmf_vb_load_posterior(self.ctx, str(path).encode()))

    def vb_timing(self):
        """Device ms of the last transpose of the tables, scoring launch, selection and guest launch."""
        return self._ms(lib.sbmf_vb_timing, "ms_transpose", "ms_score", "ms_select", "ms_guest")

    def close(self):
        if self.ctx is not None:
            lib.sbmf_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FMLearnVBOnline(FMLearnSBPMF):
    """Online variational Bayes learner (the reference's fm_learn_vb_online,
    `bin/libFM -method vb_online`; src/libfm/src/fm_learn_vb_online.h).
    ``learn(sweeps=n)`` runs n epochs of 30 mini-batches; ``rmse_trajectory``
    holds the per-epoch test RMSE of the posterior-mean prediction,
    ``factors()`` / ``biases()`` the posterior means, ``hyper()["tau"]`` alpha."""

    def __init__(self, num_factor=8, num_iter=100, seed=1, rng="ref", device=0, vb_batches=0, **kw):
        super().__init__(num_factor=num_factor, num_iter=num_iter, seed=seed, rng=rng, device=device, method="vb",
                         vb_batches=vb_batches, **kw)


def samples_file_info(path):
    """sbmf_samples_file_info: a sample file's header, validated against the file's size (no GPU):
    {"version", "precision" ("f64" | "f32"), "num_users", "num_items", "num_factor", "count", "bias", "bytes"}."""
    v = [C.c_uint32() for _ in range(7)]
    b = C.c_uint64()
    rc = lib.sbmf_samples_file_info(str(path).encode(), *[C.byref(x) for x in v], C.byref(b))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    keys = ("version", "precision", "num_users", "num_items", "num_factor", "count", "bias")
    out = {k: x.value for k, x in zip(keys, v)}
    out["precision"] = "f32" if out["precision"] == F32 else "f64"
    out["bias"] = bool(out["bias"])
    out["bytes"] = b.value
    return out


def vb_posterior_file_info(path):
    """sbmf_vb_posterior_file_info: a VB posterior file's header, validated against the file's size
    (no GPU): {"version", "num_users", "num_items", "num_factor", "bytes"}."""
    v = [C.c_uint32() for _ in range(4)]
    b = C.c_uint64()
    rc = lib.sbmf_vb_posterior_file_info(str(path).encode(), *[C.byref(x) for x in v], C.byref(b))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    out = {k: x.value for k, x in zip(("version", "num_users", "num_items", "num_factor"), v)}
    out["bytes"] = b.value
    return out


def samples_hyper_file_info(path):
    """sbmf_samples_hyper_file_info: the header of a sample file's companion file, validated against
    the file's size (no GPU): {"version", "num_factor", "count", "bytes"}."""
    v = [C.c_uint32() for _ in range(3)]
    b = C.c_uint64()
    rc = lib.sbmf_samples_hyper_file_info(str(path).encode(), *[C.byref(x) for x in v], C.byref(b))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    out = {k: x.value for k, x in zip(("version", "num_factor", "count"), v)}
    out["bytes"] = b.value
    return out


def device_usage(device=0):
    """sbmf_test_device_usage: hipMemGetInfo plus the library's live device / pinned
    buffers, streams, events, contexts and RCCL communicators (a dict)."""
    u = _lib.DeviceUsage()
    rc = lib.sbmf_test_device_usage(device, C.byref(u))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    return {f: getattr(u, f) for f, _ in u._fields_}


def tgauss(mean, sign, seed=1, it=0, mode="device", index=None, device=0):
    """sbmf_test_tgauss: the latent targets of classification for cases with the predictions
    ``mean`` and labels ``sign`` (>= 0: the positive class) -- mode "device": the Philox draw of
    the train frames at the key (seed, it, index[i] or i); mode "host": the reference's truncated
    normals over its own stream seeded with ``seed``, drawn in order (no GPU needed)."""
    mean = _f64(mean).ravel()
    sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sign, np.int32), mean.shape))
    idx = None if index is None else _u32(index).ravel()
    out = np.zeros(len(mean))
    rc = lib.sbmf_test_tgauss(0 if mode == "device" else 1, device, seed, it, len(mean), _ptr(mean, C.c_double),
                              _ptr(sg, C.c_int32), None if idx is None else _ptr(idx, C.c_uint32),
                              _ptr(out, C.c_double))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    return out



class Communicator:
    """sbmf_comm_create: one RCCL communicator for the process (ncclCommInitRank once),
    attached in turn by every learner created with ``init(comm=<this>)``."""

    def __init__(self, nranks, rank, uid, device=0):
        h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
        rc = lib.sbmf_comm_create(device, nranks, rank, buf, C.byref(h))
        if rc != SBMF_OK:
            raise SBMFError(rc, lib.sbmf_last_global_error().decode())
        self.handle, self.nranks, self.rank = h, nranks, rank

    def close(self):
        if self.handle is not None:
            lib.sbmf_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    buf = (C.c_uint8 * 128)()
    rc = lib.sbmf_comm_unique_id(buf)
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    return bytes(buf)


def ref_stream(seed, kind, n, shape=1.0):
    """Host reference stream: kind 0 rand(), 1 ran_gaussian(), 2 ran_gamma(shape)."""
    out = np.zeros(n)
    rc = lib.sbmf_ref_stream(seed, kind, shape, n, _ptr(out, C.c_double))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    return out


def partition_rows(ptr, nranks):
    """Row blocks [bounds[k], bounds[k+1]) of every rank (host-only, as the library partitions)."""
    ptr = _u32(ptr)
    out = np.zeros(nranks + 1, dtype=np.uint64)
    rc = lib.sbmf_partition_rows(_ptr(ptr, C.c_uint32), len(ptr) - 1, nranks, _ptr(out, C.c_uint64))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    return out


def philox_normals(seed, sweep, tag, row, K):
    out = np.zeros(K)
    rc = lib.sbmf_philox_normals(seed, sweep, tag, row, K, _ptr(out, C.c_double))
    if rc != SBMF_OK:
        raise SBMFError(rc, lib.sbmf_last_global_error().decode())
    return out
