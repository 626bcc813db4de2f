"""Round plans of tests/test_backend_rounds_gpu.py: which BA, PnP and DLT problems share a round of the batch engine, and which sequence
(`seq`, one set of back-end workspaces) solves which. tests/test_backend_rounds_plan.py checks on the CPU that the plans do reach the paths
they are meant to reach: the numbers come from the formulas of ba_prepare / ba_fill_prob and from the constants of the kernels' sources.

A volley is a list of N_SEQ entries; entry j is what thread j submits with seq = j. The BA volleys run in the order of BA_RUN."""
import functools
import importlib.util
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "practical-multi-view_amd", "csrc")
N_SEQ = 8


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ba_maker = _load("make_ba_chain_golden")
pnp_maker = _load("make_pnp_chain_golden")


@functools.lru_cache(maxsize=None)
def ba_problems():
    """name -> problem tuple of make_ba_chain_golden.problems()"""
    return {p[0]: p for p in ba_maker.problems()}


@functools.lru_cache(maxsize=None)
def pnp_problems():
    """name -> (obj, img, rvec_guess, tvec_guess) of make_pnp_chain_golden.problems()"""
    return {p[0]: p[1:] for p in pnp_maker.problems()}


# ---- the kernels' constants, read from their sources -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kernel_constants():
    with open(os.path.join(CSRC, "backend_ba.hip")) as f:
        ba = f.read()
    with open(os.path.join(CSRC, "backend_pnp.hip")) as f:
        pnp = f.read()
    out = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", ba).group(1)) for k in ("BM_T", "BM_PB")}
    out["BG_H"] = int(re.search(r"constexpr int BG_W = \d+, BG_H = (\d+);", ba).group(1))
    out["PNP_H0"] = int(re.search(r'getenv\("PMV_PNP_STAGE1"\) \? atoi\(getenv\("PMV_PNP_STAGE1"\)\) : (\d+);', pnp).group(1))
    return out


def _ceil(a, b):
    return (a + b - 1) // b


def ba_dims(prob):
    """what ba_prepare and ba_fill_prob derive from a problem's sizes, and the K-slices of the one-workgroup mode"""
    k = kernel_constants()
    _, cams, pts, obs, _, _, cap = prob
    nc, np_, nobs = len(cams), len(pts), len(obs)
    m = 6 * nc
    tiles_r, tiles_c = _ceil(m, 16), _ceil(m + 1, 16)
    ldw, krows = 16 * tiles_c, _ceil(3 * np_, 16) * 16
    nbo, nbp = _ceil(nobs, k["BM_T"]), _ceil(np_, k["BM_PB"])
    clear_blocks = min(64, _ceil(krows * ldw, 4 * k["BM_T"]))
    ks = min(8, max(1, 8 // (tiles_r * tiles_c)))   # multi = false
    kper = _ceil(_ceil(krows, ks), 16) * 16
    return dict(nc=nc, np=np_, nobs=nobs, cap=cap, m=m, tiles=tiles_r * tiles_c, gemm_blocks=tiles_r * tiles_c * k["BG_H"], krows=krows, ldw=ldw,
                nbo=nbo, nbp=nbp, eval_blocks=nbo + clear_blocks, ks_mode1=ks, kslices_mode1=_ceil(krows, kper))


ROUND_MAXIMA = ("eval_blocks", "nc", "nbp", "tiles", "m")   # BABatchDims: max_eval_blocks, max_nc, max_nbp, max_tiles, max_m


def holders(names, key):
    """the problems of a launch chain that set the chain's maximum of `key`"""
    d = {n: ba_dims(ba_problems()[n])[key] for n in names}
    top = max(d.values())
    return sorted(n for n, v in d.items() if v == top)


def chains(names):
    """process_ba, mode 0: one launch chain per distinct iteration cap, in the order the caps first appear"""
    caps = []
    for n in names:
        cap = ba_problems()[n][6]
        if cap not in caps:
            caps.append(cap)
    return [(cap, [n for n in names if ba_problems()[n][6] == cap]) for cap in caps]


def describe(names):
    """one line per volley: the caps in it and who holds each maximum of each launch chain"""
    parts = []
    for cap, chain in chains(names):
        parts.append(f"cap {cap} x{len(chain)}: " + ", ".join(f"max_{k} {'/'.join(holders(chain, k))}" for k in ROUND_MAXIMA))
    return "; ".join(parts)


# ---- BA ------------------------------------------------------------------------------------------------------------------------------
BA_VOLLEYS = {
    # one cap, eight shapes; max_nc / max_tiles / max_m from nc10_np300, max_nbp / max_eval_blocks from nc5_np1000
    "shapes": ["nc1_np1", "nc2_np5", "nc5_np16", "nc5_np17", "nc6_np80", "nc10_np300", "nc5_np1000", "nc5_np40_degenerate_ray"],
    # caps 1, 50, 50 and five at 5: three launch chains on D.a.d + i0
    "caps": ["nc5_np100_it1", "nc5_np100_it50", "nc5_np100_noiseless", "nc5_np100_at_the_optimum", "nc5_np120_far_start", "nc5_np60_dup_straddle",
             "nc5_np60_cam_blind_in_slice", "nc5_np390"],
    # the rest, and the smallest and the largest problems once more on other sequences
    "reuse": ["nc5_np700", "nc3_np200", "nc5_np60", "nc5_np760", "nc5_np800", "nc1_np1", "nc10_np300", "nc5_np1000"],
}
BA_VOLLEYS["shapes_reversed"] = BA_VOLLEYS["shapes"][::-1]
BA_VOLLEYS["caps_reversed"] = BA_VOLLEYS["caps"][::-1]
BA_RUN = ["shapes", "caps", "reuse", "shapes_reversed", "caps_reversed"]
# the only shapes with ks = 8 and with ks = 1 in the one-workgroup mode: never relaxed against the oracle
BA_NEVER_RELAXED = ("nc1_np1", "nc2_np5", "nc6_np80", "nc10_np300")

# Not among the golden problems. With one or two cameras the one-workgroup mode asks for ks = 8 K-slices, but the golden problems of that
# kind have 16 rows, which is one slice: these have enough rows for seven slices with a short last one, and for eight full ones.
BA_EIGHT_SLICES = {"nc2_np100": (48, 2, 100), "nc2_np128": (49, 2, 128)}   # name -> (seed, nc, np) of scenes.ba_problem, every point seen by both
BA_EIGHT_SLICES_VOLLEY = ["nc2_np100", "nc10_np300", "nc2_np128", "nc6_np80", "nc5_np390", "nc1_np1", "nc2_np100", "nc3_np200"]


@functools.lru_cache(maxsize=None)
def ba_eight_slice_problems():
    import scenes
    out = {}
    for name, (seed, nc, npts) in BA_EIGHT_SLICES.items():
        P = scenes.ba_problem(seed, nc=nc, npts=npts, vis=1.0)
        out[name] = (name, P["cams"], P["pts"], P["obs"], P["cam_idx"], P["pt_idx"], 5)
    return out


# ---- PnP: (problem, iterations, reproj_err, confidence) ------------------------------------------------------------------------------
PNP_NO_MODEL = "all_outliers_m50"
PNP_HIGH_OUTLIER = "s25_m300"


def _d(name, iterations=100, reproj_err=8.0, confidence=0.99):
    return (name, iterations, reproj_err, confidence)


PNP_GOLDEN_VOLLEYS = {   # default arguments: the recorded bits
    "golden_a": [_d(n) for n in ("s26_m6", "s24_m12", "s12_m64", "s13_m65", "s4_m217", "s25_m300", "s21_m700", "all_outliers_m50")],
    "golden_b": [_d(n) for n in ("s22_m40", "s26_m6", "all_outliers_m50", "s13_m65", "s24_m12", "s12_m64", "s22_m40", "s4_m217")],
}
PNP_MIXED_VOLLEYS = {    # no recording: the single call and the oracle at the same arguments
    # max_hyp = 1024 from the no-model problem: its pose is hypothesis 1023's, the last wavefront of the second launch
    "mixed_a": [_d("s26_m6", 1), _d("s24_m12", 8), _d("s25_m300", 16), _d("s25_m300", 17), _d("all_outliers_m50", 17), _d("all_outliers_m50", 1024),
                _d("s13_m65", 100, confidence=0.5), _d("s4_m217", 100, reproj_err=2.0)],
    # max_hyp = 1024 from s13_m65: the no-model problems' hypotheses end at 16 and 99, far below the grid of the second launch
    "mixed_b": [_d("all_outliers_m50", 17), _d("s13_m65", 1024), _d("s25_m300", 16, confidence=0.5), _d("s26_m6", 17), _d("all_outliers_m50", 100),
                _d("s21_m700", 8), _d("s22_m40", 1), _d("s12_m64", 16, reproj_err=2.0)],
}

# ---- DLT: (seed, n) of scenes.two_view_problem ------------------------------------------------------------------------------------------
DLT_VOLLEY = [(11, 1), (12, 63), (13, 64), (14, 65), (15, 400), (16, 1500), (17, 64), (18, 1)]
