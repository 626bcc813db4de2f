"""The round plans of tests/backend_rounds_common.py reach what tests/test_backend_rounds_gpu.py is there for: every golden problem, a round
whose maxima come from different problems, three iteration caps in one round, a small problem after a large one on every sequence's
workspaces, PnP hypothesis counts on both sides of the split between the two launches, unequal n in a DLT round. No device needed: the
numbers are those ba_prepare, ba_fill_prob, process_ba and launch_pnp_batch compute, from the constants in the kernels' sources."""
import backend_rounds_common as rc


def _dims(name):
    return rc.ba_dims(rc.ba_problems()[name])


def test_constants_are_read_from_the_sources():
    k = rc.kernel_constants()
    assert k["BM_T"] % 64 == 0 and k["BM_PB"] >= 1 and k["BG_H"] >= 1 and 1 <= k["PNP_H0"] < 100, k


def test_every_ba_problem_is_in_a_volley_of_eight():
    for name, volley in rc.BA_VOLLEYS.items():
        assert len(volley) == rc.N_SEQ, name
    assert set(rc.BA_RUN) == set(rc.BA_VOLLEYS)
    assert len(rc.ba_problems()) == 21
    assert set().union(*rc.BA_VOLLEYS.values()) == set(rc.ba_problems())
    for a in ("shapes", "caps"):   # the same round in the opposite order of sequences
        assert rc.BA_VOLLEYS[a + "_reversed"] == rc.BA_VOLLEYS[a][::-1]


def test_one_cap_eight_shapes_and_the_maxima_from_different_problems():
    v = rc.BA_VOLLEYS["shapes"]
    assert len(rc.chains(v)) == 1 and "nc1_np1" in v
    assert len({(_dims(n)["nc"], _dims(n)["np"], _dims(n)["nobs"]) for n in v}) == 8
    widest = rc.holders(v, "nc")
    longest = rc.holders(v, "nbp")
    assert len(widest) == 1 and len(longest) == 1 and widest != longest
    assert rc.holders(v, "tiles") == widest and rc.holders(v, "m") == widest and rc.holders(v, "eval_blocks") == longest
    # so every other problem has blocks that must leave at once in every k_bamB_* launch, and k_bamB_solve / k_ba_lm_batch get more LDS than
    # their own m asks for
    for n in v:
        d, w, l = _dims(n), _dims(widest[0]), _dims(longest[0])
        if n != widest[0]:
            assert d["nc"] < w["nc"] and d["gemm_blocks"] < w["gemm_blocks"] and d["m"] < w["m"]
        if n != longest[0]:
            assert d["nbp"] < l["nbp"] and d["eval_blocks"] < l["eval_blocks"]
    smallest = _dims("nc1_np1")
    assert (smallest["nc"], smallest["np"], smallest["nbp"], smallest["nbo"], smallest["tiles"]) == (1, 1, 1, 1, 1)


def test_three_caps_in_one_round():
    v = rc.BA_VOLLEYS["caps"]
    ch = rc.chains(v)
    assert sorted((cap, len(names)) for cap, names in ch) == [(1, 1), (5, 5), (50, 2)]
    by_cap = dict(ch)
    assert by_cap[1] == ["nc5_np100_it1"] and sorted(by_cap[50]) == ["nc5_np100_it50", "nc5_np100_noiseless"]
    assert set(by_cap[5]) == {"nc5_np100_at_the_optimum", "nc5_np120_far_start", "nc5_np60_dup_straddle", "nc5_np60_cam_blind_in_slice", "nc5_np390"}
    # two of the three chains start past the first record (D.a.d + i0, i0 > 0), whichever order the requests arrive in; within the chain
    # of five the maximum of the point blocks is one problem's alone
    assert len(rc.holders(by_cap[5], "nbp")) == 1 and _dims(rc.holders(by_cap[5], "nbp")[0])["nbp"] > _dims("nc5_np60_dup_straddle")["nbp"]


def test_every_sequence_solves_a_small_problem_after_a_large_one():
    v = rc.BA_VOLLEYS["reuse"]
    assert {"nc5_np60", "nc3_np200", "nc5_np700", "nc5_np760", "nc5_np800", "nc1_np1", "nc10_np300", "nc5_np1000"} == set(v)
    for seq in range(rc.N_SEQ):
        nps = [_dims(rc.BA_VOLLEYS[name][seq])["np"] for name in rc.BA_RUN]
        drops = [(a, b) for a, b in zip(nps, nps[1:]) if a >= 300 and 4 * b <= a]
        assert drops, f"seq {seq} solves np = {nps}: never a problem a quarter the size of the one before on the same workspaces"
    # the smallest and the largest problems run on two different sequences
    for n in ("nc1_np1", "nc10_np300", "nc5_np1000"):
        assert rc.BA_VOLLEYS["shapes"].index(n) != rc.BA_VOLLEYS["reuse"].index(n)


def test_one_workgroup_mode_sees_every_slice_count():
    ks = {n: _dims(n)["ks_mode1"] for n in rc.ba_problems()}
    assert {n for n, k in ks.items() if k == 8} == {"nc1_np1", "nc2_np5"}
    assert {n for n, k in ks.items() if k == 1} == {"nc6_np80", "nc10_np300"}
    assert all(k == 2 for n, k in ks.items() if n not in rc.BA_NEVER_RELAXED)
    assert set(rc.BA_NEVER_RELAXED) <= set(rc.BA_VOLLEYS["shapes"])   # all three counts in ONE round, whose LDS is sized by nc10_np300's m
    # a problem of one point has fewer rows than slices: one short slice
    assert _dims("nc1_np1")["kslices_mode1"] == 1 and _dims("nc2_np5")["kslices_mode1"] == 1 and _dims("nc3_np200")["kslices_mode1"] == 2


def test_eight_slices_in_the_one_workgroup_mode():
    d = {n: rc.ba_dims(p) for n, p in rc.ba_eight_slice_problems().items()}
    assert all(v["ks_mode1"] == 8 and v["np"] == rc.BA_EIGHT_SLICES[n][2] for n, v in d.items())
    assert d["nc2_np100"]["kslices_mode1"] == 7 and d["nc2_np100"]["krows"] % 7 != 0   # kper = 48: six full slices and one of 16 rows
    assert d["nc2_np128"]["kslices_mode1"] == 8 and d["nc2_np128"]["krows"] == 8 * 48
    v = rc.BA_EIGHT_SLICES_VOLLEY
    assert len(v) == rc.N_SEQ and set(rc.BA_EIGHT_SLICES) <= set(v) and set(v) <= set(rc.BA_EIGHT_SLICES) | set(rc.ba_problems())
    assert {"nc10_np300", "nc6_np80", "nc3_np200"} <= set(v)   # ks = 1 and 2 in the same round


def test_pnp_plans():
    h0 = rc.kernel_constants()["PNP_H0"]
    names = set(rc.pnp_problems())
    assert len(names) == 9 and rc.PNP_NO_MODEL in names and rc.PNP_HIGH_OUTLIER in names
    for volley in list(rc.PNP_GOLDEN_VOLLEYS.values()) + list(rc.PNP_MIXED_VOLLEYS.values()):
        assert len(volley) == rc.N_SEQ and all(r[0] in names for r in volley)
    a, b = rc.PNP_GOLDEN_VOLLEYS["golden_a"], rc.PNP_GOLDEN_VOLLEYS["golden_b"]
    assert all(r[1:] == (100, 8.0, 0.99) for r in a + b)
    assert len({r[0] for r in a}) == 8 and {r[0] for r in a} | {r[0] for r in b} == names
    assert {"s26_m6", "s25_m300", "s13_m65", "s21_m700", rc.PNP_NO_MODEL} <= {r[0] for r in a}
    mixed = rc.PNP_MIXED_VOLLEYS["mixed_a"]
    assert {r[1] for r in mixed} == {1, 8, 16, 17, 100, 1024}
    assert {r[1] for r in mixed if r[0] == rc.PNP_NO_MODEL} == {17, 1024} and {r[1] for r in mixed if r[0] == rc.PNP_HIGH_OUTLIER} == {16, 17}
    assert [r[3] for r in mixed].count(0.5) == 1 and [r[2] for r in mixed].count(2.0) == 1
    for volley in rc.PNP_MIXED_VOLLEYS.values():   # counts below, at, one above and far above the split, so max_hyp > h0: two launches
        its = [r[1] for r in volley]
        assert min(its) < h0 and h0 in its and h0 + 1 in its and max(its) > h0 + 1
        assert any(r[0] == rc.PNP_NO_MODEL and r[1] > h0 for r in volley), "no no-model pose from the second launch"
    # who sets the round's max_hyp: the no-model problem in mixed_a, another one in mixed_b
    top = lambda volley: {r[0] for r in volley if r[1] == max(q[1] for q in volley)}
    assert top(rc.PNP_MIXED_VOLLEYS["mixed_a"]) == {rc.PNP_NO_MODEL}
    assert rc.PNP_NO_MODEL not in top(rc.PNP_MIXED_VOLLEYS["mixed_b"]) and any(r[0] == rc.PNP_NO_MODEL for r in rc.PNP_MIXED_VOLLEYS["mixed_b"])


def test_dlt_plan():
    ns = [n for _, n in rc.DLT_VOLLEY]
    assert len(ns) == rc.N_SEQ and set(ns) == {1, 63, 64, 65, 400, 1500} and ns.count(max(ns)) == 1
    assert len({seed for seed, _ in rc.DLT_VOLLEY}) == rc.N_SEQ
