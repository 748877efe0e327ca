"""The two half-batch lanes stay apart across calls and are joined on demand: a halves run leaves the side
stream open, and whatever uses the context's stream next joins it first.  Every case runs the same calls on a context with
set_half_batches(False) -- one stream, nothing to join -- and compares what download() returns.

What is compared (_assert_same): the result records byte for byte, and EVERY element of matches / mask / points / point_idx.
In the rows a record counts (n_matches, n_points) the bytes are equal.  Behind the counts an element is either equal too, or
untouched on both contexts -- the same bytes as in the download taken before the first run: matches, points and point_idx
are not cleared when a batch is created, so what no run writes is whatever the allocation held, on one stream as on two.  A
stray write of the other lane behind a count fails either way.  Against a batch with another history (a fresh one, a lone
run) the counted rows are compared, and of a record without a model its counts and residual (see _assert_same).

Shape: 65 pairs (halves of 33 and 32; 64 is the threshold), 256 keypoints, 2048 hypotheses, Philox, threshold 1e-2.  In the
ragged fixtures one half is all empty pairs, so that half's lane runs far ahead of the other lane's tail."""
import functools
import os
import re

import numpy as np
import pytest

from mvslam_amd import synth

P, N, H, THR = 65, 256, 2048, 1e-2
HALF = (P + 1) // 2
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvslam_amd", "csrc")


def _capi():
    from mvslam_amd import capi
    return capi


@functools.lru_cache(maxsize=None)
def _data(kind, first=700):
    """uniform: every pair full; first_empty / second_empty: the pairs of that half have no keypoints"""
    d = synth.make_batch(first, P, n_kp=N)
    n1, n2 = d["n1"].copy(), d["n2"].copy()
    if kind == "first_empty":
        n1[:HALF], n2[:HALF] = 0, 0
    elif kind == "second_empty":
        n1[HALF:], n2[HALF:] = 0, 0
    else:
        assert kind == "uniform"
    d = dict(d, n1=n1, n2=n2)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


KINDS = ("uniform", "first_empty", "second_empty")


def _prm(seed=91, thr=THR, hyp=H):
    capi = _capi()
    return capi.default_params(num_hypotheses=hyp, sampler=capi.SAMPLER_PHILOX, seed=seed, max_error_sq=thr)


ARRAYS = ("matches", "mask", "points", "point_idx")


def _batch(ctx, data, count=P):
    """a batch with `data` resident; b.pre: its output arrays before any run"""
    b = _capi().Batch(ctx, count, N, 32)
    _upload(b, data)
    b.pre = b.download()
    return b


def _out(b):
    out = b.download()
    out["pre"] = b.pre
    return out


def _upload(b, data):
    b.upload(0, data["desc1"], data["kp1"], data["n1"], data["desc2"], data["kp2"], data["n2"], data["K"], data["global_index"])


def _elements(x):
    """[pair][row][bytes of one element]"""
    x = np.ascontiguousarray(x)
    return x.view(np.uint8).reshape(x.shape[0], x.shape[1], -1)


def _assert_same(a, b, count=None, same_history=True):
    """same_history: a and b come from the same calls on two contexts (see the module's docstring).  Otherwise b comes from a
    batch that held nothing else before: the counted rows are compared, and the records where they are valid -- a run rewrites
    the counts and the residual of every record (its first 32 bytes) but the model fields (F ... t) only where it found a
    model, so a pair that has none keeps those of an earlier upload's run, on one stream as on two."""
    res = a["results"]
    count = len(res) if count is None else count
    if same_history:
        assert a["results"][:count].tobytes() == b["results"][:count].tobytes()
    else:
        for i in range(count):
            n = res.itemsize if res["valid"][i] else 32
            assert a["results"][i].tobytes()[:n] == b["results"][i].tobytes()[:n], ("results", i)
    for k in ARRAYS:
        for i in range(count):
            n = int(res["n_matches"][i]) if k in ("mask", "matches") else int(res["n_points"][i])
            assert a[k][i][:n].tobytes() == b[k][i][:n].tobytes(), (k, i)
        if same_history:
            equal = (_elements(a[k]) == _elements(b[k])).all(-1)
            untouched = ((_elements(a[k]) == _elements(a["pre"][k])).all(-1) & (_elements(b[k]) == _elements(b["pre"][k])).all(-1))
            bad = np.argwhere(~(equal | untouched))
            assert len(bad) == 0, (k, bad[:4].tolist())


@pytest.fixture(scope="module")
def lanes():
    """(two lanes, one stream): the first context's stream is never handed out, so its halves runs leave the lane open"""
    capi = _capi()
    on, off = capi.Context(0), capi.Context(0)
    off.set_half_batches(False)
    yield on, off
    on.close()
    off.close()


def _both(lanes, fn):
    """fn(ctx) on the two-lane context and on the one-stream context"""
    return fn(lanes[0]), fn(lanes[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_five_runs_without_sync(lanes, kind):
    def go(ctx):
        b = _batch(ctx, _data(kind))
        for _ in range(5):
            b.run(_prm())
        out = _out(b)
        b.close()
        return out

    _assert_same(*_both(lanes, go))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_second_parameters_equal_a_lone_run(lanes, kind):
    prm_a, prm_b = _prm(), _prm(seed=17, thr=1e-3)

    def go(ctx):
        b = _batch(ctx, _data(kind))
        b.run(prm_a)
        b.run(prm_b)
        out = _out(b)
        b.close()
        return out

    def lone(ctx):
        b = _batch(ctx, _data(kind))
        b.run(prm_b)
        out = _out(b)
        b.close()
        return out

    two, one = _both(lanes, go)
    _assert_same(two, one)
    _assert_same(two, lone(lanes[1]), same_history=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_upload_behind_an_open_lane(lanes, kind):
    other = _data({"uniform": "uniform", "first_empty": "second_empty", "second_empty": "first_empty"}[kind], first=900)

    def go(ctx):
        b = _batch(ctx, _data(kind))
        b.run(_prm())
        _upload(b, other)
        b.run(_prm())
        out = _out(b)
        b.close()
        return out

    def fresh(ctx):
        b = _batch(ctx, other)
        b.run(_prm())
        out = _out(b)
        b.close()
        return out

    two, one = _both(lanes, go)
    _assert_same(two, one)
    _assert_same(two, fresh(lanes[1]), same_history=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_one_stream_run_behind_an_open_lane(lanes, kind):
    def go(ctx):
        b = _batch(ctx, _data(kind))
        b.run(_prm())
        b.run(_prm(seed=5), n_active=40)   # below the threshold: the one-stream path, over pairs of both halves
        out = _out(b)
        b.close()
        return out

    _assert_same(*_both(lanes, go))


@pytest.mark.gpu
def test_two_batches_interleaved(lanes):
    def go(ctx):
        a, b = _batch(ctx, _data("first_empty")), _batch(ctx, _data("second_empty"))
        for _ in range(2):
            a.run(_prm())
            b.run(_prm(seed=3))
        outs = _out(a), _out(b)
        a.close()
        b.close()
        return outs

    two, one = _both(lanes, go)
    _assert_same(two[0], one[0])
    _assert_same(two[1], one[1])


FOLLOW_UPS = ("refine", "stats", "time_kernel", "time_total", "copy_results_device", "download_async", "batch_close", "ctx_close")


@pytest.mark.gpu
@pytest.mark.parametrize("what", FOLLOW_UPS)
def test_follow_up_joins_the_open_lane(lanes, what):
    """run() without sync, then one call of every kind that uses the context's stream.  first_empty: the main lane is idle
    at once, so a follow-up that did not join would run beside the second half."""
    capi = _capi()
    data = _data("first_empty")

    def go(ctx, halves):
        if what == "ctx_close":   # a context of its own to close
            ctx = capi.Context(0)
            ctx.set_half_batches(halves)
        b = _batch(ctx, data)
        b.run(_prm())
        got = None
        if what == "refine":
            b.refine()
            r = b.download_refined(points=True, point_cov=True)
            # the refinement skips a pair without a model and leaves its record as allocated: the records of the valid pairs
            valid = b.download(matches=False, mask=False, points=False)["results"]["valid"] != 0
            assert valid[HALF:].any()
            got = r["refined"][valid].tobytes() + r["points"][valid].tobytes() + r["point_cov"][valid].tobytes()
        elif what == "stats":
            got = repr(sorted(b.stats(_prm()).items())).encode()
        elif what in ("time_kernel", "time_total"):
            total, kern = b.time(_prm(), steps=2, warmup=1, per_kernel=what == "time_kernel")
            assert np.isfinite(total) and total > 0.0
            assert what == "time_total" or all(np.isfinite(v) and v > 0.0 for v in kern.values())
        elif what == "copy_results_device":
            dstb = capi.Batch(ctx, P, N, 32)   # device memory to copy into: another batch's (zeroed) records
            b.copy_results_device(dstb.results_device()[0])
            b.sync()
            got = dstb.download(matches=False, mask=False, points=False)["results"].tobytes()
            dstb.close()
        elif what == "download_async":
            res = capi.pinned_empty((P,), capi.RESULT_DTYPE)
            mk = capi.pinned_empty((P, N), np.uint8)
            b.download_async(0, P, res, mask=mk)
            b.sync()
            n = res["n_matches"].astype(int)
            got = res.tobytes() + b"".join(mk[i][:n[i]].tobytes() for i in range(P))
            capi.pinned_free(res)
            capi.pinned_free(mk)
        elif what == "batch_close":
            b.close()
            return None, None
        elif what == "ctx_close":
            ctx.close()   # closes the batch, then the context, behind the open lane
            return None, None
        out = _out(b)
        b.close()
        return got, out

    two, one = go(lanes[0], True), go(lanes[1], False)
    assert two[0] == one[0]
    if two[1] is not None:
        _assert_same(two[1], one[1])


@pytest.mark.gpu
def test_tables_grow_behind_an_open_lane(lanes):
    def go(ctx):
        b = _batch(ctx, _data("first_empty"))
        b.run(_prm())
        b.run(_prm(hyp=40000))   # the per-hypothesis tables are reallocated: the second half must have left them
        out = _out(b)
        b.close()
        return out

    _assert_same(*_both(lanes, go))


@pytest.mark.gpu
def test_caller_on_the_stream_sees_both_halves():
    """The eager path: a caller who can enqueue on the context's stream (they read it, or it is theirs: a borrowed torch
    stream) sees one stream -- a torch op enqueued on it right behind run() reads the finished records of both halves.  In
    a process of its own (tests/lane_join_torch_check.py), because torch brings its own HIP runtime and has to be the first
    to load one."""
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "lane_join_torch_check.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream_read ok" in r.stdout and "borrowed ok" in r.stdout, r.stdout


@pytest.mark.gpu
def test_sequence_run_halves_on_and_off(lanes):
    capi = _capi()
    F = 70
    seq = synth.make_sequence(F, n_kp=N)

    def go(ctx):
        s = capi.Sequence(ctx, F, N, 32)
        s.upload(0, seq["desc"][:F], seq["kp"][:F], seq["n_kp"][:F], seq["K"])
        pre = s.download_pairs()
        s.run(_prm(), capi.default_pnp_params(num_hypotheses=100, seed=7, reproj_error=2.0))
        pairs, tracks = dict(s.download_pairs(), pre=pre), s.download_tracks()
        s.close()
        return pairs, tracks

    two, one = _both(lanes, go)
    _assert_same(two[0], one[0])
    tr = two[1]["tracks"]
    assert tr.tobytes() == one[1]["tracks"].tobytes()
    for k, cnt in (("corr_xyz", "n_corr"), ("corr_uv", "n_corr"), ("inlier_idx", "n_inliers")):   # rows the records count
        for i in range(len(tr)):
            n = int(tr[cnt][i])
            assert two[1][k][i][:n].tobytes() == one[1][k][i][:n].tobytes(), (k, i)


def _function_spans(text, names):
    """line ranges of the top-level functions `names` of a source text: from the line that names one to the next '}' in
    column 0"""
    lines = text.split("\n")
    spans = []
    for name in names:
        for i, ln in enumerate(lines):
            if re.match(r"^\w[\w\s\*:]*\b%s\(" % re.escape(name), ln) and not ln.rstrip().endswith(";"):
                j = next(k for k in range(i, len(lines)) if lines[k] == "}")
                spans.append((i, j))
    return spans


def test_the_streams_are_read_in_one_place():
    """From the source text: outside the accessor (ctx_stream), the join (close_lane), the halves path (enqueue_pipeline) and
    the context's create / destroy / stream getter nothing names the context's two streams."""
    raw = re.compile(r"(->|\.)(stream|side)\b")
    allowed = {"capi.hip": ("close_lane", "enqueue_pipeline", "mvs_ctx_create_on_stream", "mvs_ctx_destroy"),
               "capi_internal.hpp": ("ctx_stream",), "capi_orb.hip": (), "capi_graph.hip": (), "capi_debug.hip": ()}
    for name, fns in allowed.items():
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        spans = _function_spans(text, fns)
        assert len(spans) == len(fns), (name, spans)
        for i, ln in enumerate(text.split("\n")):
            code = ln.split("//")[0]
            if raw.search(code) and "lt->" not in code and "lt." not in code:
                assert any(a <= i <= b for a, b in spans), "%s:%d: %s" % (name, i + 1, ln.strip())
