"""The front half of the `sbmf` command line -- everything before the context is created: which message
a command line gets, which of two applicable messages wins, and the errors of every list file
(-rec_users, -rec_guests, -rec_queries, <stem>.queries, -rec_exclude).  No GPU is needed: every list
file is parsed before sbmf_create, so a row that passes all parsers ends at "no HIP device" on a
host without one (on a GPU host those rows are skipped: the run itself is test_gpu_cli's).

The expectations were recorded from the binary of the commit before the command line was split into
stages (built from a worktree of that commit), and are asserted as whole ERROR lines."""
import subprocess

import numpy as np
import pytest

from conftest import gpu_available
from sbmf._lib import CLI_PATH

F = ["-task", "r", "-train", "nope/train", "-test", "nope/test"]  # flags alone: neither file exists
C = ["-task", "c"] + F[2:]
T = ["-task", "r", "-train", "tr.tsv", "-test", "te.tsv"]  # triples
L = ["-task", "r", "-train", "tr.libfm", "-test", "te.libfm"]  # libFM text, users 0..2, items 3..4
U = T + ["-recommend", "top.txt", "-rec_users"]
G = T + ["-recommend_guests", "top.txt", "-rec_guests"]
Q = L + ["-method", "als", "-relation", "relu,reli", "-recommend_queries", "top.txt", "-rec_relation", "reli"]
QQ = Q + ["-rec_queries", "q.libfm"]
RECQ = ["-recommend_queries", "x", "-rec_queries", "q", "-rec_relation", "a"]

TASK = "only -task r (regression) is supported by the SBPMF sampler"
REC = "-recommend is offered by the SBPMF sampler (-method mcmc -order sbpmf)"
RECG = ("-recommend_guests is offered by the SBPMF sampler (-method mcmc -order sbpmf) with the unbiased quirk sets "
        "(final, sbpmf2, none)")
RECQ_NO = ("-recommend_queries is offered by libFM's MCMC / ALS learner (-method mcmc -order libfm, -method als) with "
           "-relation: it ranks the block rows of one relation")
GO_REC = "-rec_users / -rec_topn / -rec_risk go with -recommend"
GO_RECQ = "-rec_queries / -rec_relation / -rec_exclude go with -recommend_queries <file>"
TOPN = "-rec_topn must be in 1..1024"
REL = ("-relation: block-structure relations are drawn by libFM's MCMC / ALS learner (-method mcmc -order libfm, "
       "-method als); %s does not read them, and without them the relations' features would be missing")
GENERAL = ("the input holds cases that are not one user and one item feature; %s: use -method mcmc (libFM order) or "
           "-method als on such a file")
REGULAR = "-regular takes 'r', 'r0,r1,r2'%s; 2 given"
NOTE = "note: -order sbpmf: bias terms (k0,k1) are not sampled"
DEVICE = object()  # the row passes every parser: "no HIP device" on a host without one


def flags(id, args, err):
    """decided by the flags alone: no file is opened, nothing is loaded"""
    return dict(id=id, args=args, err=err, flags_only=True)


def row(id, args, err, files=None, **kw):
    return dict(id=id, args=args, err=err, files=files or {}, **kw)


ROWS = [
    # ---- flags alone
    flags("c_vb", C + ["-method", "vb"], TASK),
    flags("c_sbpmf", C + ["-order", "sbpmf"], TASK),
    flags("c_quirks_without_order", C + ["-quirks", "final"], TASK),
    flags("c_triple", C + ["-format", "triple"], TASK),
    flags("task_missing", F[2:], TASK),
    flags("recommend_no_name", F + ["-recommend", "-rec_users", "u"], "-recommend needs a file name"),
    flags("recommend_guests_no_name", F + ["-recommend_guests", "-rec_guests", "g"], "-recommend_guests needs a file name"),
    flags("recommend_queries_no_name", F + ["-recommend_queries", "-rec_queries", "q"],
          "-recommend_queries needs a file name"),
    flags("recommend_no_users", F + ["-recommend", "x"], "-recommend needs -rec_users <file> (one user id per line)"),
    flags("recommend_guests_no_guests", F + ["-recommend_guests", "x"],
          "-recommend_guests needs -rec_guests <file> ('guest item rating' per line)"),
    flags("recommend_queries_no_queries", F + ["-recommend_queries", "x"],
          "-recommend_queries needs -rec_queries <file> (the queries in libFM text format)"),
    flags("recommend_queries_no_relation", F + ["-recommend_queries", "x", "-rec_queries", "q"],
          "-recommend_queries needs -rec_relation <stem> (one of -relation's stems)"),
    flags("rec_users_alone", F + ["-rec_users", "u"], GO_REC),
    flags("rec_users_with_guests_only", F + ["-recommend_guests", "x", "-rec_guests", "g", "-rec_users", "u"], GO_REC),
    flags("rec_guests_alone", F + ["-rec_guests", "g"], "-rec_guests goes with -recommend_guests <file>"),
    flags("rec_queries_alone", F + ["-rec_queries", "q"], GO_RECQ),
    flags("rec_relation_alone", F + ["-rec_relation", "a"], GO_RECQ),
    flags("rec_exclude_alone", F + ["-rec_exclude", "e"], GO_RECQ),
    flags("rec_topn_alone", F + ["-rec_topn", "3"], GO_REC),
    flags("rec_risk_alone", F + ["-rec_risk", "1"], GO_REC),
    flags("queries_vb", F + ["-method", "vb", "-relation", "a"] + RECQ, RECQ_NO),
    flags("queries_no_relation", F + ["-method", "als"] + RECQ, RECQ_NO),
    flags("queries_unknown_stem", F + ["-method", "als", "-relation", "relu,reli"] + RECQ[:4] + ["-rec_relation", "items"],
          "-rec_relation items names none of -relation's stems (relu,reli)"),
    flags("recommend_als", F + ["-method", "als", "-recommend", "x", "-rec_users", "u"], REC),
    flags("recommend_guests_vb", F + ["-method", "vb", "-recommend_guests", "x", "-rec_guests", "g"], RECG),
    flags("topn_0_users", F + ["-recommend", "x", "-rec_users", "u", "-rec_topn", "0"], TOPN),
    flags("topn_1025_users", F + ["-recommend", "x", "-rec_users", "u", "-rec_topn", "1025"], TOPN),
    flags("topn_0_guests", F + ["-recommend_guests", "x", "-rec_guests", "g", "-rec_topn", "0"], TOPN),
    flags("topn_1025_guests", F + ["-recommend_guests", "x", "-rec_guests", "g", "-rec_topn", "1025"], TOPN),
    flags("topn_0_queries", F + ["-method", "als", "-relation", "a"] + RECQ + ["-rec_topn", "0"], TOPN),
    flags("topn_1025_queries", F + ["-method", "als", "-relation", "a"] + RECQ + ["-rec_topn", "1025"], TOPN),
    flags("topn_not_a_number", F + ["-recommend", "x", "-rec_users", "u", "-rec_topn", "abc"], TOPN),
    flags("format_unknown", F + ["-format", "csv"], "unknown -format csv"),
    # which of two faults is reported
    flags("task_before_missing_rec_users", C + ["-method", "vb", "-recommend", "x"], TASK),
    flags("queries_vb_before_unknown_stem", F + ["-method", "vb", "-relation", "a"] + RECQ[:4] + ["-rec_relation", "zz"],
          RECQ_NO),
    flags("recommend_als_before_topn", F + ["-method", "als", "-recommend", "x", "-rec_users", "u", "-rec_topn", "0"], REC),
    flags("topn_before_format", F + ["-recommend", "x", "-rec_users", "u", "-rec_topn", "0", "-format", "csv"], TOPN),
    flags("missing_rec_users_before_stray_rec_guests", F + ["-recommend", "x", "-rec_guests", "g"],
          "-recommend needs -rec_users <file> (one user id per line)"),
    # ---- after the train file is sniffed (triples: -order sbpmf; libFM text: -order libfm)
    row("order_unknown", T + ["-order", "foo"], "unknown -order foo"),
    row("c_on_triples", ["-task", "c"] + T[2:], TASK),
    row("relation_sbpmf", L + ["-relation", "relu", "-order", "sbpmf"], REL % "-method mcmc -order sbpmf (the SBPMF sampler)"),
    row("relation_vb", L + ["-relation", "relu", "-method", "vb"], REL % "-method vb (online VB)"),
    row("relation_on_triples", T + ["-relation", "relu"], REL % "-method mcmc -order sbpmf (the SBPMF sampler)"),
    row("recommend_libfm_default_order", L + ["-recommend", "x", "-rec_users", "users.txt"], REC),
    row("queries_sbpmf", L + ["-order", "sbpmf", "-relation", "relu"] + RECQ[:4] + ["-rec_relation", "relu"],
        REL % "-method mcmc -order sbpmf (the SBPMF sampler)"),
    row("guests_bias2", T + ["-quirks", "bias2", "-recommend_guests", "x", "-rec_guests", "g"], RECG),
    row("guests_libfm_order", L + ["-recommend_guests", "x", "-rec_guests", "g"], RECG),
    row("method_sgd", T + ["-method", "sgd"], "-method sgd is not supported (use mcmc, als or vb)"),
    row("order_before_method", T + ["-method", "sgd", "-order", "foo"], "unknown -order foo"),
    row("test_missing", T[:4], "-train and -test are mandatory"),
    row("dim_two_numbers", T + ["-dim", "1,1"], "dim must have 3 numbers", note=None),
    row("dim_k2_zero", T + ["-dim", "1,1,0"], "dim k2 must be in [1,256]"),
    row("dim_vb", T + ["-method", "vb", "-dim", "0,0,8"],
        "the online VB learner updates w0 and the user/item w: use -dim '1,1,K'"),
    row("als_bias2", L + ["-method", "als", "-quirks", "bias2"],
        "-quirks bias2|bias22 selects the SBPMF biased sampler, not libFM's"),
    row("bias2_dim", T + ["-quirks", "bias2", "-dim", "0,0,8"],
        "the biased sampler (gibbs_sbpmf2.cpp) samples b0 and the user/item biases: use -dim '1,1,K'", note=None),
    row("average_unknown", T + ["-average", "foo"], "unknown -average foo"),
    row("quirks_unknown", T + ["-quirks", "foo"], "unknown -quirks foo"),
    row("dim_before_average", T + ["-dim", "1,1", "-average", "foo"], "dim must have 3 numbers"),
    row("note_sbpmf_k0_k1", T + ["-dim", "1,1,8"], DEVICE, note=NOTE, out="Loading test"),
    row("note_then_average", T + ["-dim", "0,1,8", "-average", "foo"], "unknown -average foo", note=NOTE),
    row("no_note_without_k0_k1", T + ["-dim", "0,0,8"], DEVICE, note=None, out="Loading test"),
    # ---- loading
    row("general_recommend", ["-task", "r", "-train", "gen.libfm", "-test", "gen.libfm", "-order", "sbpmf", "-recommend", "x",
                              "-rec_users", "users.txt"],
        GENERAL % "-recommend / -recommend_guests rank the items of the SBPMF sampler's user x item model", out="Loading test"),
    row("general_vb", ["-task", "r", "-train", "gen.libfm", "-test", "gen.libfm", "-method", "vb"],
        GENERAL % "-method vb (online VB) updates one user and one item attribute per case"),
    row("general_sbpmf", ["-task", "r", "-train", "gen.libfm", "-test", "gen.libfm", "-order", "sbpmf", "-dim", "0,0,8"],
        GENERAL % "-order sbpmf (the SBPMF sampler) factorizes a user x item rating matrix"),
    row("train_unopenable", ["-task", "r", "-train", "nope/train", "-test", "te.tsv"], "unable to open nope/train", out="Loading train"),
    row("regular_count", L + ["-regular", "1,2"], REGULAR % " (1 + 2G values need the G groups of a -meta file)"),
    row("regular_count_meta", L + ["-meta", "meta.txt", "-regular", "1,2"],
        REGULAR % " or, with the 2 groups of -meta, 5 values 'r0,w_lambda[g]..,v_lambda[g]..'"),
    row("meta_short", L + ["-meta", "meta_short.txt"],
        "-meta: meta_short.txt holds 2 group ids; 6 attributes need one each (entry 3 is missing)"),
    row("relation_unloadable", L + ["-relation", "relbad"], "-relation relbad: unable to open relbad.xt (or .x)"),
    row("relations_load", L + ["-relation", "relu,reli"], DEVICE, out="#relations: 2"),
    # ---- -rec_users
    row("users_unopenable", U + ["nope.txt"], "Unable to open file nope.txt", out="Loading test"),
    row("users_not_a_number", U + ["u.txt"], "-rec_users: cannot read a user id from ' x1'", files={"u.txt": "0\n x1\n"}),
    row("users_too_large", U + ["u.txt"], "-rec_users: cannot read a user id from '4294967295'",
        files={"u.txt": "4294967295\n"}),
    row("users_only_comments", U + ["u.txt"], "-rec_users: u.txt lists no user", files={"u.txt": "# nobody\n\n \t\n"}),
    row("users_blank_and_comment_lines", U + ["users.txt"], DEVICE),
    # ---- -rec_guests
    row("guests_unopenable", G + ["nope.txt"], "Unable to open file nope.txt"),
    row("guests_two_fields", G + ["g.txt"], "-rec_guests: cannot read 'guest item rating' from '0 1'",
        files={"g.txt": "0 0 5\n0 1\n"}),
    row("guests_decreasing", G + ["g.txt"], "-rec_guests: guest numbers must not decrease ('0 1 3')",
        files={"g.txt": "1 0 5\n0 1 3\n"}),
    row("guests_decreasing_before_item_range", L + ["-order", "sbpmf", "-dim", "0,0,8", "-recommend_guests", "top.txt",
                                                    "-rec_guests", "g.txt"],
        "-rec_guests: guest numbers must not decrease ('0 1 3')", files={"g.txt": "1 3 5\n0 1 3\n"}),
    row("guests_item_below_offset", L + ["-order", "sbpmf", "-dim", "0,0,8", "-recommend_guests", "top.txt", "-rec_guests",
                                         "g.txt"],
        "-rec_guests: item id out of range in '0 2 4'", files={"g.txt": "0 3 5\n0 2 4\n"}),
    row("guests_item_at_offset", L + ["-order", "sbpmf", "-dim", "0,0,8", "-recommend_guests", "top.txt", "-rec_guests",
                                      "g.txt"], DEVICE, files={"g.txt": "0 3 5\n0 4 4\n"}),
    row("guests_none", G + ["g.txt"], "-rec_guests: g.txt lists no guest", files={"g.txt": "# nobody\n\n"}),
    row("guests_skipped_number", G + ["g.txt"], DEVICE, files={"g.txt": "# two guests, one without ratings\n0 0 5\n\n2 1 3\n"}),
    # ---- -rec_queries and <stem>.queries
    row("queries_loader_error", Q + ["-rec_queries", "qbad.libfm"], "-rec_queries: cannot parse libFM line 1 of qbad.libfm",
        files={"qbad.libfm": "1 0:1 x\n"}),
    row("queries_unopenable", Q + ["-rec_queries", "nope.libfm"], "-rec_queries: unable to open nope.libfm"),
    row("queries_empty", Q + ["-rec_queries", "qempty.libfm"], "-rec_queries: qempty.libfm lists no query",
        files={"qempty.libfm": ""}),
    row("stem_queries_missing", QQ, "Unable to open file relu.queries"),
    row("stem_queries_not_a_number", QQ, "relu.queries: cannot read a block row from 'two'",
        files={"relu.queries": "0\ntwo\n"}),
    row("stem_queries_count", QQ, "relu.queries holds 3 block rows; -rec_queries 2 queries",
        files={"relu.queries": "0\n# a comment\n1\n2\n"}),
    row("stem_queries_ok", QQ, DEVICE, files={"relu.queries": "0\n\n2\n"}),
    # ---- -rec_exclude
    row("exclude_unopenable", QQ + ["-rec_exclude", "nope.txt"], "Unable to open file nope.txt",
        files={"relu.queries": "0\n2\n"}),
    row("exclude_one_field", QQ + ["-rec_exclude", "e.txt"], "-rec_exclude: cannot read 'query row' from '1'",
        files={"relu.queries": "0\n2\n", "e.txt": "0 1\n1\n"}),
    row("exclude_query_number_at_n", QQ + ["-rec_exclude", "e.txt"], "-rec_exclude: query number out of range in '2 0'",
        files={"relu.queries": "0\n2\n", "e.txt": "0 1\n2 0\n"}),
    row("exclude_decreasing", QQ + ["-rec_exclude", "e.txt"], "-rec_exclude: query numbers must not decrease ('0 2')",
        files={"relu.queries": "0\n2\n", "e.txt": "1 1\n0 2\n"}),
    row("exclude_lists_nothing", QQ + ["-rec_exclude", "e.txt"], DEVICE,
        files={"relu.queries": "0\n2\n", "e.txt": "# nothing\n"}),
    row("exclude_ok", QQ + ["-rec_exclude", "e.txt"], DEVICE, files={"relu.queries": "0\n2\n", "e.txt": "1 0\n1 2\n"}),
    row("exclude_without_name", QQ + ["-rec_exclude"], DEVICE, files={"relu.queries": "0\n2\n"}),
]


def write_inputs(d):
    """The tiny inputs every row finds in its working directory."""
    import sbmf
    (d / "tr.tsv").write_text("0\t0\t5\n1\t1\t3\n0\t1\t4\n2\t0\t1\n")
    (d / "te.tsv").write_text("1\t0\t2\n2\t1\t4\n")
    (d / "tr.libfm").write_text("5 0:1 3:1\n3 1:1 4:1\n4 0:1 4:1\n1 2:1 3:1\n")
    (d / "te.libfm").write_text("2 1:1 3:1\n4 2:1 4:1\n")
    (d / "gen.libfm").write_text("5 0:1 3:1 5:0.5\n3 1:1\n")
    (d / "meta.txt").write_text("0\n0\n0\n1\n1\n1\n")  # users 0..2, items 3..4 and libFM's one id beyond
    (d / "meta_short.txt").write_text("0\n0\n")
    (d / "users.txt").write_text("# the watched users\n\n  0\n2\r\n")
    (d / "q.libfm").write_text("0 0:1\n0 2:1 4:1\n")
    # two relations of three block rows over the 4 train and 2 test cases
    block = sbmf.Cases([0, 1, 3, 4], [0, 0, 1, 2], [1, 1, 0.5, 1], np.zeros(3))
    sbmf.save_libfm_relation(str(d / "relu"), sbmf.Relation(block, [0, 1, 0, 2], [1, 2]))
    sbmf.save_libfm_relation(str(d / "reli"), sbmf.Relation(block, [0, 1, 1, 0], [0, 1], group=[0, 0, 1]))


def _param(r):
    device = r["err"] is DEVICE
    marks = [pytest.mark.skipif(gpu_available(), reason="the run itself is test_gpu_cli's")] if device else []
    return pytest.param(r, id=r["id"], marks=marks)


@pytest.mark.parametrize("r", [_param(r) for r in ROWS])
def test_front(r, tmp_path):
    write_inputs(tmp_path)
    for name, text in r.get("files", {}).items():
        (tmp_path / name).write_text(text)
    p = subprocess.run([CLI_PATH, *r["args"]], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    errors = [l for l in p.stderr.splitlines() if l.startswith("ERROR:")]
    assert p.returncode == 1 and len(errors) == 1 and p.stderr.splitlines()[-1] == errors[0], p.stderr
    if r["err"] is DEVICE:
        assert "no HIP device" in errors[0]
    else:
        assert errors[0] == "ERROR: " + r["err"]
    if r.get("flags_only"):
        assert "open" not in p.stderr.lower() and "Loading" not in p.stdout
    if "note" in r:  # the stderr note of -order sbpmf with k0 or k1 set: printed once, or (None) not at all
        notes = [l for l in p.stderr.splitlines() if l.startswith("note:")]
        assert (len(notes) == 1 and notes[0].startswith(r["note"])) if r["note"] else not notes
    if r.get("out"):
        assert r["out"] in p.stdout
    assert not (tmp_path / "top.txt").exists()  # no output file before the run
