"""The consumer entries behind the path (include/amcx.h: amcx_group_stats_f32 / _ws_f32, amcx_standardize_fit_transform_f32,
amcx_select_scale_f32, amcx_mlp_classify_f32) on the host: their refusals in the order the header states -- limits, the
workspace's size, the no-op, then every pointer's null, alignment and device check through one list -- and the launch layer's
claim that every kernel goes through it.  No call below is a valid one on host memory: each is refused, or has nothing to do.
Needs no GPU."""
import ctypes as C
from pathlib import Path

from amcpy_amd import _lib
from tests.stream_inputs import aligned as _aligned

REPO = Path(__file__).resolve().parents[1]
E, OK = _lib.EINVAL, _lib.OK
# the row gate's products past 2^58 (each factor in range on its own), as tests/test_occupancy_host.py's gather test
PAST_2_58 = ((1 << 40, 1 << 40), (1 << 2, (1 << 56) + 1))


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


STATS_LIMITS = (dict(G=-1), dict(G=1 << 31), dict(R=0), dict(R=-1), dict(C=0), dict(C=33, stride=33), dict(stride=17), dict(stride=0),
                dict(stride=-18), dict(stride=(1 << 20) + 1))


def test_group_stats_ws_refusals_in_the_documented_order_without_a_device():
    lib = _lib.load()
    f = lib.amcx_group_stats_ws_f32
    keep, p = _aligned()
    need = lib.amcx_group_stats_workspace_bytes(3, 10, 18)
    assert need > 0
    nul = dict(x=None, mean=None, std=None, ws=None)

    def call(**kw):
        a = {**dict(x=p, G=3, R=10, stride=18, C=18, mean=p, std=p, ws=p, wsb=need), **kw}
        return f(a["x"], a["G"], a["R"], a["stride"], a["C"], a["mean"], a["std"], a["ws"], a["wsb"], None)
    # 1. ranges and strides, also where the call would otherwise be the no-op
    for kw in STATS_LIMITS:
        assert call(**kw) == E and call(**{"G": 0, **nul, **kw}) == E, kw
    # 2. the workspace's size
    assert call(wsb=need - 1) == E and call(wsb=0) == E and call(wsb=-1) == E
    # 3. nothing to do: no pointer is looked at
    assert call(G=0, wsb=0, **nul) == OK and call(G=0, R=1 << 40, C=32, stride=1 << 20, wsb=0, **nul) == OK
    # 4. null pointers and alignment, every pointer of the entry
    for kw in (dict(x=None), dict(mean=None), dict(std=None), dict(ws=None),
               dict(x=p + 2), dict(mean=p + 4), dict(std=p + 4), dict(ws=p + 4)):
        assert call(**kw) == E, kw
    del keep


def test_group_stats_refusals_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_group_stats_f32
    keep, p = _aligned()
    nul = dict(x=None, mean=None, std=None)

    def call(**kw):
        a = {**dict(x=p, G=3, R=10, stride=18, C=18, mean=p, std=p), **kw}
        return f(a["x"], a["G"], a["R"], a["stride"], a["C"], a["mean"], a["std"], None)
    for kw in STATS_LIMITS:
        assert call(**kw) == E and call(**{"G": 0, **nul, **kw}) == E, kw
    assert call(G=0, **nul) == OK and call(G=0, R=1 << 40, C=32, stride=1 << 20, **nul) == OK
    # (the entry's own workspace is asked for behind these: a refused call allocates nothing)
    for kw in (dict(x=None), dict(mean=None), dict(std=None), dict(x=p + 2), dict(mean=p + 4), dict(std=p + 4)):
        assert call(**kw) == E, kw
    del keep


def test_standardize_refusals_in_the_documented_order_without_a_device():
    lib = _lib.load()
    f = lib.amcx_standardize_fit_transform_f32
    keep, p = _aligned()
    need = lib.amcx_standardize_workspace_bytes(100, 18)
    assert need > 0
    nul = dict(x=None, out=None, mean=None, scale=None, ws=None)

    def call(**kw):
        a = {**dict(x=p, R=100, stride=18, C=18, cols=_i32(2, 4, 6), n_sel=3, out=p, ostride=3, mean=p, scale=p, ws=p, wsb=need), **kw}
        return f(a["x"], a["R"], a["stride"], a["C"], a["cols"], a["n_sel"], a["out"], a["ostride"], a["mean"], a["scale"], a["ws"],
                 a["wsb"], None)
    # 1. ranges and strides, also where the call would otherwise be the no-op
    for kw in (dict(R=-1), dict(n_sel=0), dict(n_sel=-1), dict(n_sel=33), dict(C=0), dict(C=33, stride=33), dict(cols=None),
               dict(cols=_i32(2, 4, 18)), dict(cols=_i32(-1, 4, 6)), dict(stride=17), dict(stride=0), dict(stride=-18), dict(ostride=2),
               dict(ostride=0), dict(ostride=-3)):
        assert call(**kw) == E and call(**{"R": 0, **nul, **kw}) == E, kw
    # ... the products with the row count, the statistics' stride limit and the transform's grid: where there are rows
    for R, s in PAST_2_58:
        assert call(R=R, stride=s) == E and call(R=R, ostride=s) == E, (R, s)
    assert call(stride=(1 << 20) + 1) == E and call(R=1 << 41) == E
    assert call(R=0, stride=1 << 50, ostride=1 << 60, wsb=0, **nul) == OK     # no row, no product
    # 2. the workspace's size
    assert call(wsb=need - 1) == E and call(wsb=0) == E and call(wsb=-1) == E
    # 3. nothing to do: no pointer is looked at
    assert call(R=0, wsb=0, **nul) == OK and call(R=0, C=32, stride=32, cols=_i32(*range(32)), n_sel=32, ostride=32, wsb=0, **nul) == OK
    # 4. null pointers and alignment, every pointer of the entry
    for kw in (dict(x=None), dict(out=None), dict(mean=None), dict(scale=None), dict(ws=None),
               dict(x=p + 2), dict(out=p + 2), dict(mean=p + 4), dict(scale=p + 4), dict(ws=p + 4)):
        assert call(**kw) == E, kw
    del keep


def test_select_scale_refusals_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_select_scale_f32
    keep, p = _aligned()
    nul = dict(x=None, cols=None, mean=None, scale=None, out=None)

    def call(**kw):
        a = {**dict(x=p, R=100, stride=18, cols=p, n_sel=3, mean=p, scale=p, out=p, ostride=3), **kw}
        return f(a["x"], a["R"], a["stride"], a["cols"], a["n_sel"], a["mean"], a["scale"], a["out"], a["ostride"], None)
    # 1. ranges and strides, also where the call would otherwise be the no-op
    for kw in (dict(R=-1), dict(n_sel=0), dict(n_sel=-1), dict(stride=0), dict(stride=-18), dict(ostride=2), dict(ostride=0),
               dict(ostride=-3)):
        assert call(**kw) == E and call(**{"R": 0, **nul, **kw}) == E, kw
    # the row gate on either side: a product with the row count past 2^58
    for R, s in PAST_2_58:
        assert call(R=R, stride=s) == E and call(R=R, ostride=s) == E, (R, s)
    assert call(R=0, stride=1 << 60, ostride=1 << 60, **nul) == OK            # no row, no product
    # 2. nothing to do: no pointer is looked at
    assert call(R=0, **nul) == OK and call(R=0, n_sel=1 << 30, ostride=1 << 30, **nul) == OK
    # 3. null pointers and alignment, every pointer of the entry
    for kw in (dict(x=None), dict(cols=None), dict(mean=None), dict(scale=None), dict(out=None),
               dict(x=p + 2), dict(cols=p + 2), dict(mean=p + 4), dict(scale=p + 4), dict(out=p + 2)):
        assert call(**kw) == E, kw
    del keep


def test_mlp_classify_refusals_in_the_documented_order_without_a_device():
    f = _lib.load().amcx_mlp_classify_f32
    keep, p = _aligned()
    w = _i32(6, 26, 29, 30, 6)
    nul = dict(x=None, mean=None, scale=None, params=None, labels=None, probs=None, counts=None)

    def call(**kw):
        a = {**dict(x=p, n_rows=1000, stride=18, n_cols=18, cols=_i32(2, 4, 6, 8, 12, 14), n_sel=6, mean=p, scale=p, params=p, widths=w,
                    n_linear=4, act=_lib.ACT_RELU, labels=p, probs=p, pstride=6, rpg=100, counts=p), **kw}
        return f(a["x"], a["n_rows"], a["stride"], a["n_cols"], a["cols"], a["n_sel"], a["mean"], a["scale"], a["params"], a["widths"],
                 a["n_linear"], a["act"], a["labels"], a["probs"], a["pstride"], a["rpg"], a["counts"], None)
    # 1. the limits, also where the call would otherwise be the no-op (a stride or a group is judged where its pointer is given)
    for kw in (dict(n_rows=-1), dict(n_cols=0), dict(n_cols=33, stride=33), dict(stride=17), dict(stride=0), dict(stride=-18),
               dict(cols=None), dict(widths=None), dict(widths=_i32(6, 0, 29, 30, 6)), dict(widths=_i32(6, 33, 29, 30, 6)),
               dict(n_linear=0), dict(widths=_i32(*[6] * 8), n_linear=7), dict(n_sel=5, cols=_i32(2, 4, 6, 8, 12)), dict(act=3),
               dict(act=-1), dict(mean=None, scale=p), dict(mean=p, scale=None), dict(cols=_i32(2, 4, 6, 8, 12, 18)),
               dict(cols=_i32(-1, 4, 6, 8, 12, 14)), dict(probs=p, pstride=5), dict(probs=p, pstride=0), dict(probs=p, pstride=-6),
               dict(rpg=-1), dict(rpg=0, counts=p)):
        assert call(**kw) == E and call(**{"n_rows": 0, **nul, **kw}) == E, kw
    # ... and where there are rows: whole groups, and the products with the row count past 2^58
    assert call(rpg=999) == E and call(n_rows=0, rpg=999, **nul) == OK
    for R, s in PAST_2_58:
        assert call(n_rows=R, stride=s, rpg=0, counts=None) == E and call(n_rows=R, pstride=s, rpg=0, counts=None) == E, (R, s)
    assert call(**{**nul, "probs": p}, n_rows=0, stride=1 << 60, pstride=1 << 60) == OK                # no row, no product
    # 2. nothing to do: no pointer is looked at
    assert call(n_rows=0, **nul) == OK and call(n_rows=0, rpg=0, **nul) == OK
    # 3. null pointers (x and the parameters: every output is optional, mean and scale go together) and alignment, every pointer
    for kw in (dict(x=None), dict(params=None), dict(x=p + 2), dict(mean=p + 4), dict(scale=p + 4), dict(params=p + 2),
               dict(labels=p + 2), dict(probs=p + 2), dict(counts=p + 4)):
        assert call(**kw) == E, kw
    # 4. no output asked for: AMCX_OK behind the pointer checks, nothing launched
    none = dict(labels=None, probs=None, counts=None, rpg=0)
    assert call(**none) == OK and call(**none, mean=None, scale=None) == OK
    assert call(**none, x=None) == E and call(**none, params=None) == E and call(**none, x=p + 2) == E and call(**none, mean=p + 4) == E
    del keep


def test_every_kernel_is_launched_through_the_launch_layer():
    """amcx_launch.h's opening sentence: hipLaunchKernelGGL stands in amcx::launch, and in the FMA probe's timed lambda it names."""
    hits = {f.name: f.read_text().count("hipLaunchKernelGGL(") for f in sorted((REPO / "amcpy_amd" / "csrc").iterdir()) if f.is_file()}
    assert {k: v for k, v in hits.items() if v} == {"amcx_launch.h": 1, "amcx_probe.h": 1}
    text = (REPO / "amcpy_amd" / "csrc" / "amcx.hip").read_text()
    assert "AMCX_HIP(hipGetLastError())" not in text                         # every launch's error carries the launch's name
