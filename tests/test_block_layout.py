"""The staging blocks' layouts (csrc/backend_layout.h) and the cursor that carves them (csrc/pmv_block.h), checked on the host.

tests/twin/block_layout_check.cpp includes the two headers alone and prints every offset and size; it is compiled twice with g++, once plain
and once with -fsanitize=address,undefined, and run as a program. Here every printed number is compared with the formula the back-end used
before the layouts had one home, written out literally:

  (a) every offset and size of every call kind's layout, and the sizes of the blocks at capacity;
  (b) whatever a call with n <= max_tracks carves fits each block it is carved from;
  (c) the cursor: takes never overlap, honour their alignment, a dry run agrees with a real one, and a take past the capacity raises the
      overflow flag and hands out no pointer.

One size differs from the earlier formula on purpose. d_tri_in, which the DLT and the five-point round share, was sized by the DLT alone:
384 + 33 * max_tracks + 64 bytes. A five-point round of FP_MAX_HYP samples over n points needs 32 n + 1280, so where max_tracks < 832 a round
over more than (33 * max_tracks - 896) / 32 points (40 of 64) was refused with PMV_ERR_CAPACITY although pmv_fivepoint_hypotheses admits
n <= max_tracks. The block is now the larger of the two needs (+ 64); from max_tracks = 832 on, the benchmark's 4096 included, nothing
changes. test_capacity_sizes pins both numbers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW = os.path.join(ROOT, "tests", "twin")
CSRC = os.path.join(ROOT, "practical-multi-view_amd", "csrc")
NS = (0, 1, 5, 15, 63, 64, 2000)
MAX_HYP, FP_MAX_HYP, PNP_HDR, ESS_HDR, ESS_OUT_HDR = 1024, 64, 384, 64, 128
SMALL, METRIC = (64, 4, 32, 96), (4096, 32, 8192, 65536)   # (max_tracks, max_ba_cams, max_ba_points, max_ba_obs)


def a64(x):
    return (x + 63) & ~63


def _records(sanitize):
    exe = os.path.join(TW, "block_layout_check_asan" if sanitize else "block_layout_check")
    srcs = [os.path.join(TW, "block_layout_check.cpp"), os.path.join(CSRC, "pmv_block.h"), os.path.join(CSRC, "backend_layout.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in srcs):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", CSRC, srcs[0], "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    recs = {}
    for line in out.splitlines():
        kind, *kv = line.split()
        recs.setdefault(kind, []).append({k: (v if k in ("kind", "run") else int(v)) for k, v in (x.split("=") for x in kv)})
    return out, recs


@pytest.fixture(scope="module")
def recs():
    plain_out, plain = _records(False)
    san_out, _ = _records(True)   # the same program under the sanitizers: it ends clean and prints the same
    assert san_out == plain_out
    return plain


def _one(recs, kind, **key):
    hit = [r for r in recs[kind] if all(r[k] == v for k, v in key.items())]
    assert len(hit) == 1, (kind, key, len(hit))
    return hit[0]


def test_constants(recs):
    assert recs["const"] == [dict(MAX_HYP=1024, FP_MAX_HYP=64, PNP_HDR=384, ESS_HDR=64, ESS_OUT_HDR=128, PNP_OUT_INFO=48, PNP_OUT_DONE=60, PNP_OUT_INLIERS=64,
                                  ESS_OUT_INFO=80, ESS_OUT_DONE=92, BA_SUM_SLOTS=8, BA_SUM_DONE=7)]


@pytest.mark.parametrize("m", NS)
@pytest.mark.parametrize("it", (1, MAX_HYP))
def test_pnp_layout(recs, m, it):
    in_bytes = PNP_HDR + m * 20 + it * 20
    ho = a64(in_bytes)
    assert _one(recs, "pnp", m=m, it=it) == dict(m=m, it=it, K=0, obj=PNP_HDR, img=PNP_HDR + 12 * m, samples=PNP_HDR + 20 * m, in_bytes=in_bytes, out=ho,
                                                 info=ho + 48, done=ho + 60, inliers=ho + 64, total=ho + 64 + 4 * m)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("h", (1, FP_MAX_HYP))
def test_fivepoint_layout(recs, n, h):
    in_bytes = 4 * n * 8 + 5 * h * 4
    ho = a64(in_bytes)
    assert _one(recs, "fivepoint", n=n, h=h) == dict(n=n, h=h, q1=0, q2=16 * n, samples=32 * n, in_bytes=in_bytes, out=ho, models=ho, n_models=ho + h * 90 * 8,
                                                     counts=ho + h * 90 * 8 + h * 4, total=ho + h * (90 * 8 + 44))


@pytest.mark.parametrize("n", NS)
def test_dlt_layout(recs, n):
    in_bytes = (48 + 4 * n) * 8 + n
    ho = a64(in_bytes)
    assert _one(recs, "dlt", n=n) == dict(n=n, P=0, q1=48 * 8, q2=48 * 8 + 16 * n, mask_in=48 * 8 + 32 * n, in_bytes=in_bytes, out=ho, Q=ho, mask=ho + 16 * n * 8,
                                          total=ho + 16 * n * 8 + 4 * n)


@pytest.mark.parametrize("n", NS)
def test_whole_ransac_layouts(recs, n):
    in_bytes = ESS_HDR + (5 * n + 2) * 8
    ho = a64(in_bytes)
    assert _one(recs, "essential", n=n) == dict(n=n, rec=0, p1=ESS_HDR, p2=ESS_HDR + 16 * n, iters=ESS_HDR + 32 * n, in_bytes=in_bytes, out=ho, info=ho + 80,
                                                done=ho + 92, mask=ho + ESS_OUT_HDR, total=ho + ESS_OUT_HDR + n)
    in_bytes = ESS_HDR + n * 16 + (n + 2) * 8
    ho = a64(in_bytes)
    assert _one(recs, "fundamental", n=n) == dict(n=n, rec=0, p1=ESS_HDR, p2=ESS_HDR + 8 * n, iters=ESS_HDR + 16 * n, in_bytes=in_bytes, out=ho, info=ho + 80,
                                                  done=ho + 92, mask=ho + ESS_OUT_HDR, total=ho + ESS_OUT_HDR + n)


def _ba_want(nc, np_, no):
    cams = 8 * 8
    pts = cams + nc * 6 * 8
    obs = pts + np_ * 3 * 8
    K = obs + no * 2 * 8
    ci = K + 10 * 8
    pi = ci + 4 * no
    pstart = pi + 4 * no
    plist = pstart + 4 * (np_ + 1)
    cstart = plist + 4 * no
    clist = cstart + 4 * (nc + 1)
    erec = (clist + 4 * no + 15) & ~15
    return dict(nc=nc, np=np_, no=no, summary=0, cams=cams, pts=pts, obs=obs, K=K, cam_idx=ci, pt_idx=pi, pstart=pstart, plist=plist, cstart=cstart, clist=clist,
                erec=erec, io_bytes=erec + 16 * no, done=7 * 8, out_bytes=(8 + nc * 6 + np_ * 3) * 8, total=erec + 16 * no)


@pytest.mark.parametrize("no", NS)
def test_ba_io_layout(recs, no):
    for nc in (1, 4, 32):
        for np_ in (1, 5, 63):
            assert _one(recs, "ba", nc=nc, np=np_, no=no) == _ba_want(nc, np_, no)
    for _, nc, np_, no_ in (SMALL, METRIC):
        assert _one(recs, "ba", nc=nc, np=np_, no=no_) == _ba_want(nc, np_, no_)


def _parent_caps(mt, nc, np_, no):
    """backend_alloc's formulas as they stood before backend_caps"""
    n = 6 * nc + 3 * np_
    ba_io = (8 + nc * 6 + np_ * 3 + no * 2 + 10) * 8 + (no * 8 + np_ + nc + 8) * 4 + 128
    pnp_in, pnp_out = PNP_HDR + mt * 20 + MAX_HYP * 20 + 64, 48 + 16 + mt * 4 + 64
    tri_in, tri_out = 48 * 8 + mt * 32 + mt + 64, mt * 16 * 8 + mt * 4 + 64
    ess_in = ESS_HDR + (5 * mt + 2) * 8 + 64
    fund_in = ESS_HDR + mt * 24 + 16 + 64
    h_stage = max(no * 18 * 8 + no * 2 * 8, n * 8 + no * 32 + (np_ + nc + 2) * 4, mt * 32 + MAX_HYP * 20 + 4096, ba_io, pnp_in + pnp_out, tri_in + tri_out,
                  tri_in + FP_MAX_HYP * (90 * 8 + 44) + 256, ess_in + ESS_OUT_HDR + mt + 64)
    return dict(ba_io=ba_io, pnp_in=pnp_in, pnp_out=pnp_out, tri_in=tri_in, tri_out=tri_out, ess_in=ess_in, fund_in=fund_in, h_stage=h_stage)


def test_capacity_sizes(recs):
    keys = ("mt", "nc", "np", "no")
    metric = _one(recs, "caps", **dict(zip(keys, METRIC)))
    assert {k: v for k, v in metric.items() if k not in keys} == _parent_caps(*METRIC)
    small = _one(recs, "caps", **dict(zip(keys, SMALL)))
    want = _parent_caps(*SMALL)
    assert want["tri_in"] == 2560 and want["h_stage"] == 51712
    # the one departure (module docstring): d_tri_in also holds a full five-point round, and the staging block's five-point term follows it
    want["tri_in"] = max(want["tri_in"], 32 * 64 + 20 * FP_MAX_HYP + 64)
    want["h_stage"] = max(want["h_stage"], want["tri_in"] + FP_MAX_HYP * (90 * 8 + 44) + 256)
    assert want["tri_in"] == 3392 and want["h_stage"] == 52544
    assert {k: v for k, v in small.items() if k not in keys} == want


@pytest.mark.parametrize("ctx", (SMALL, METRIC), ids=("small", "metric"))
def test_every_legal_call_fits_its_blocks(recs, ctx):
    mt = ctx[0]
    caps = _one(recs, "caps", mt=mt)
    fits = [r for r in recs["fit"] if r["mt"] == mt]
    in_block = dict(pnp="pnp_in", fivepoint="tri_in", dlt="tri_in", essential="ess_in", fundamental="fund_in", ba="ba_io")
    seen = set()
    for r in fits:
        assert r["in"] <= caps[in_block[r["kind"]]], r
        assert r["total"] <= caps["h_stage"], r
        if r["kind"] == "pnp":
            assert r["out"] <= caps["pnp_out"], r   # (the device copy of the result block)
        seen.add((r["kind"], r["n"], r["k"]))
    for n in range(mt + 1):   # nothing left out: every n, both ends of the second argument
        assert {("pnp", n, 1), ("pnp", n, MAX_HYP), ("fivepoint", n, 1), ("fivepoint", n, FP_MAX_HYP), ("dlt", n, 0), ("essential", n, 0), ("fundamental", n, 0)} <= seen
    assert ("ba", 0, 0) in seen


def test_carve(recs):
    dry = [r for r in recs["carve"] if r["run"] == "dry"]
    real = [r for r in recs["carve"] if r["run"] == "real"]
    assert len(dry) == len(real) == 12
    cap = 248
    for d, r in zip(dry, real):
        assert (d["i"], d["size"], d["align"], d["off"], d["bytes"]) == (r["i"], r["size"], r["align"], r["off"], r["bytes"])   # the two runs agree
        assert d["h"] == d["d"] == -1 and d["overflow"] == 0                                                                   # a dry run hands out nothing, never overflows
        assert r["off"] % r["align"] == 0
        if r["off"] + r["size"] <= cap:
            if r["i"] != 8:   # (8 is the skip_to)
                assert r["h"] == r["d"] == r["off"]   # host and device side in step
            assert r["overflow"] == 0
        else:
            assert r["h"] == r["d"] == -1 and r["overflow"] == 1   # past the capacity: no pointer, the flag is up and stays up
        assert r["bytes"] >= r["off"] + r["size"]
    spans = sorted((r["off"], r["off"] + r["size"]) for r in real if r["size"])
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, "two takes overlap"
    assert [r["overflow"] for r in real] == [0] * 10 + [1, 1]
    assert real[9]["off"] + real[9]["size"] == cap   # a take that ends exactly at the capacity is served
