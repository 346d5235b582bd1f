"""Every NTT pass kernel instantiation (csrc/ntt.hip) at the smallest size that reaches it, as SMI_NTT_PLAN_<L> overrides.

  plan_table()                      every (logr, logw) of SMI_NTT_SHAPES (parsed from csrc/ntt_host.h, never typed in again) in
                                    every role -- first, last, middle, first with its twiddles deferred -- and one four-pass plan
  SETTINGS                          the context knobs (read when a context is created) and the families each setting runs
  legs(family, env)                 the transforms every plan of a family runs under a setting
  predicted_kernels(...)            the kernel names the profile must record for one leg
  expected(oracle, out_dir)         CPU oracle only: SHA-256 digests of every expected column, written as manifest.json
  run(manifest, report, ...)        GPU only: every leg through smi_dev_ntt, compared with the digests (or, above 2^20
                                    points, columns 1..4 with the same setting's single-column runs), kernel names recorded

Not a test module: imported by tests/test_ntt_matrix_host.py, tests/test_emu_kernels.py and tests/test_gpu_ntt_matrix.py, and
started by the last as `python tests/ntt_matrix.py MANIFEST.json REPORT.json --families=a,b` in one fresh child per
setting.  Exit status: 0 every leg equal, 1 a mismatch, 2 a call raised (the run ends at the first one)."""
import hashlib
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, G = 998244353, 3
P2, G2 = 469762049, 3
PRIMES = {"ref": (P, G, 23), "p2": (P2, G2, 26)}   # name: modulus, generator, two-adicity
COLS_PER_WG, COLS_MIN_WGS = 4, 1024                # SMI_COLS_PER_WG, SMI_COLS_MIN_WGS of csrc/ntt_core.h
BATCH = 6                                          # one full column group and a partial one
ORACLE_ALL_COLUMNS_TO = 20                         # above: columns 0 and 5 meet the oracle, 1..4 the single-column runs
GAP, SENTINEL = 64, 123456789                      # out_stride = n + GAP; the gaps keep SENTINEL (below both moduli)
FAMILIES = ("first", "last", "middle", "deferred-first", "four-pass")
INVALID_PLAN = (18, "9.3,9.3,9.3")                 # the digits sum to 27: ntt_plan_valid refuses it, the default plan runs


# --------------------------------------------------------------------------------------------------- the table
def shapes():
    """the (logr, logw) pairs of SMI_NTT_SHAPES, in the macro's order"""
    with open(os.path.join(ROOT, "stark_rs_amd", "csrc", "ntt_host.h")) as f:
        text = f.read()
    m = re.search(r"#define SMI_NTT_SHAPES\(X\)((?:.*\\\n)*.*\n)", text)
    assert m, "SMI_NTT_SHAPES not found in csrc/ntt_host.h"
    out = [(int(a), int(b)) for a, b in re.findall(r"\bX\((\d+),\s*(\d+)\)", m.group(1))]
    assert out and len(set(out)) == len(out)
    return out


def parse_plan(plan):
    return [tuple(int(v) for v in part.split(".")) for part in plan.split(",")]


def plan_valid(L, passes, kernels):
    """ntt_plan_valid of csrc/ntt_host.h: two to four passes of instantiated shapes whose digits sum to L, every strided
    pass with at least as many sub-problems left as its tile has lines, the first digit no smaller than the last tile's lines"""
    if not 2 <= len(passes) <= 4 or any(s not in kernels for s in passes) or sum(lr for lr, _ in passes) != L:
        return False
    consumed = 0
    for lr, lw in passes[:-1]:
        consumed += lr
        if L - consumed < lw:
            return False
    return passes[0][0] >= passes[-1][1]


def _s(shape):
    return "%d.%d" % shape


def plan_table():
    """-> [{"id", "family", "shape", "role", "L", "plan", "primes"}]: `shape` in `role` is what the plan is there for"""
    rows = []

    def add(family, shape, role, L, plan, primes=("ref", "p2")):
        assert sum(lr for lr, _ in parse_plan(plan)) == L
        rows.append({"id": "%s:%s@%d" % (family, _s(shape), L), "family": family, "shape": shape, "role": role, "L": L,
                     "plan": plan, "primes": tuple(k for k in primes if L <= PRIMES[k][2])})

    for s in shapes():
        lr = s[0]
        six = s == (6, 6)
        add("first", s, "first", 13 if six else lr + 6, "6.6,7.5" if six else _s(s) + ",6.6")
        add("last", s, "last", 13 if six else lr + 6, "7.5,6.6" if six else "6.6," + _s(s))
        add("middle", s, "mid", 12 + lr, "6.6,%s,6.6" % _s(s))
        add("deferred-first", s, "first", 12 + lr, "%s,6.6,6.6" % _s(s))
    add("four-pass", (6, 6), "mid", 24, "6.6,6.6,6.6,6.6", primes=("p2",))
    return rows


def _env(**kn):
    return {"SMI_NTT_" + k: str(v) for k, v in kn.items()}


# (id, environment of the child, families)
SETTINGS = [
    ("defaults", {}, ("first", "last", "middle", "four-pass")),
    ("SHARE_COLS=2-DEFER_TW=0", _env(SHARE_COLS=2, DEFER_TW=0), ("last", "middle", "four-pass")),
    ("SHARE_COLS=2-DEFER_TW=1", _env(SHARE_COLS=2, DEFER_TW=1), ("middle", "deferred-first", "four-pass")),
    ("SHARE_COLS=2-DEFER_TW=1-TWIN_REGS=0", _env(SHARE_COLS=2, DEFER_TW=1, TWIN_REGS=0), ("middle",)),
    ("SHARE_COLS=0-DEFER_TW=1-LAST_DIRECT=0", _env(SHARE_COLS=0, DEFER_TW=1, LAST_DIRECT=0), ("last", "middle", "deferred-first")),
    ("SHARE_COLS=2-LAST_DIRECT=0", _env(SHARE_COLS=2, LAST_DIRECT=0), ("last",)),
]
KNOBS = sorted({k for _, env, _ in SETTINGS for k in env})
ZLOGS = (0, 1, 2, 3, 4, 6)   # n_in = n >> z: the zlog 0 / 2 / 3 / 4 loads (1 takes the zlog 0 load, 6 the zlog 4 one)


def share_mode(env):
    v = env.get("SMI_NTT_SHARE_COLS")
    return 1 if v is None else 0 if int(v) == 0 else 2 if int(v) == 2 else 1


def legs(family, env):
    """the transforms of one plan: name -> {"batch", "inverse", "offset", "post", "nin": (shift, add) for n_in = (n >> shift) + add,
    "strided", "inplace"}"""
    def leg(batch, inverse, offset, post=1, nin=(0, 0), strided=False, inplace=False):
        return {"batch": batch, "inverse": inverse, "offset": offset, "post": post, "nin": nin, "strided": strided, "inplace": inplace}
    out = {"inv1": leg(1, True, 3, 5),                 # a scale ratio != 1: the running-product ratios of the driver matter
           "fwd1": leg(1, False, 5, nin=(3, 0))}
    if family == "first":
        for z in ZLOGS:
            if z != 3:                                 # z = 3 is fwd1
                out["fwd1_z%d" % z] = leg(1, False, 5, nin=(z, 0))
        out["fwd1_ragged-3"] = leg(1, False, 5, nin=(3, -3))
        out["fwd1_ragged+1"] = leg(1, False, 5, nin=(3, 1))
        out["fwd1_offset1"] = leg(1, False, 1, nin=(3, 0))   # no pre-scale
    if share_mode(env) == 2:
        out["inv6"] = leg(BATCH, True, 3, 5)
        out["fwd6"] = leg(BATCH, False, 5, nin=(3, 0))
        out["fwd6_strided"] = leg(BATCH, False, 5, nin=(3, 0), strided=True)
        out["inv6_inplace"] = leg(BATCH, True, 3, 5, inplace=True)
    return out


def n_in_of(leg, n):
    return (n >> leg["nin"][0]) + leg["nin"][1]


def predicted_kernels(plan, L, leg, env):
    """{kernel name: launches} of one leg: shape and role of each pass, `cols` exactly where the launcher's rule holds
    (HipLauncher::takes_cols: never a first pass, more than one column, a pass with output multipliers -- every middle pass,
    a last pass with an output scale -- and under mode 1 enough workgroups)"""
    passes, mode, batch = parse_plan(plan), share_mode(env), leg["batch"]
    out = {}
    for i, (lr, lw) in enumerate(passes):
        role = "first" if i == 0 else "last" if i == len(passes) - 1 else "mid"
        has_mul = role == "mid" or (role == "last" and leg["inverse"])
        wgs = ((1 << L) >> (lr + lw)) * ((batch + COLS_PER_WG - 1) // COLS_PER_WG)
        cols = role != "first" and mode != 0 and batch > 1 and has_mul and (mode == 2 or wgs >= COLS_MIN_WGS)
        name = "ntt_pass%s_kernel<%d,%d,%s>" % ("_cols" if cols else "", lr, lw, role)
        out[name] = out.get(name, 0) + 1
    return out


def entries(families, primes=("ref", "p2")):
    """(row of the table, prime name), the rows of `families` in the order run() takes them: by prime and size"""
    rows = [(r, k) for r in plan_table() if r["family"] in families for k in r["primes"] if k in primes]
    return sorted(rows, key=lambda rk: (rk[1], rk[0]["L"], rk[0]["id"]))


# ------------------------------------------------------------------------------------------------ inputs, expectations
def _splitmix64(seed, n):
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def column(p, L, c):
    """column c of the six: 0, 1, 3, 4 pseudo-random, 2 alternating p - 1 / 0, 5 all p - 1 (the lazy sums at their bound)"""
    n = 1 << L
    if c == 5:
        return np.full(n, p - 1, dtype=np.uint64)
    if c == 2:
        return np.where(np.arange(n) % 2 == 0, p - 1, 0).astype(np.uint64)
    return _splitmix64(0x4E5454000 + 64 * L + c, n) % np.uint64(p)


def oracle_columns(L):
    return tuple(range(BATCH)) if L <= ORACLE_ALL_COLUMNS_TO else (0, BATCH - 1)


def key(prime, L, leg, c):
    n = 1 << L
    if leg["inverse"]:
        return "%s/%d/inv/%d/%d/%d" % (prime, L, leg["offset"], leg["post"], c)
    return "%s/%d/fwd/%d/%d/%d" % (prime, L, leg["offset"], n_in_of(leg, n), c)


def oracle_column(o, prime, L, leg, c):
    """what column c of `leg` must be: fast_intt (and poly_scale for the post_scale) or fast_coset_ntt of the oracle"""
    p, g, _ = PRIMES[prime]
    n = 1 << L
    w = o.ff_prim_nth_root_g(n, p, g)
    x = column(p, L, c)
    if not leg["inverse"]:
        return o.fast_coset_ntt(x[:n_in_of(leg, n)], n, w, leg["offset"], p)
    coef = o.fast_intt(x, w, leg["offset"], p)
    if leg["post"] == 1:
        return coef
    out = np.zeros(n, dtype=np.uint64)   # so_poly_scale trims trailing zeros: what it leaves unwritten is zero
    o.lib().so_poly_scale(p, o._p(coef), n, leg["post"], o._p(out))
    return out


def digest(values):
    return hashlib.sha256(np.ascontiguousarray(values, dtype=np.uint32).tobytes()).hexdigest()


def needed_keys():
    """key -> (prime, L, leg, column) of every expectation any setting asks for"""
    need = {}
    for _, env, families in SETTINGS:
        for row, prime in entries(families):
            for leg in legs(row["family"], env).values():
                for c in ((0,) if leg["batch"] == 1 else oracle_columns(row["L"])):
                    need.setdefault(key(prime, row["L"], leg, c), (prime, row["L"], leg, c))
    row = {"L": INVALID_PLAN[0]}
    for leg in legs("middle", {}).values():
        need.setdefault(key("ref", row["L"], leg, 0), ("ref", row["L"], leg, 0))
    return need


def expected(o, out_dir, threads=16):
    """-> the manifest {"digests": {key: sha256}, "oracle_seconds"}, also written to out_dir/manifest.json"""
    from concurrent.futures import ThreadPoolExecutor
    t0 = time.time()
    need = needed_keys()
    order = sorted(need, key=lambda k: -need[k][1])   # the largest transforms first
    # the oracle's C calls release the interpreter lock and share nothing but the message of a panic, which none raises
    with ThreadPoolExecutor(threads) as pool:
        got = list(pool.map(lambda k: digest(oracle_column(o, *need[k])), order))
    man = {"digests": dict(zip(order, got)), "oracle_seconds": round(time.time() - t0, 1)}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(man, f)
    return man


# ----------------------------------------------------------------------------------------------------- GPU half
class _Group:
    """the buffers of one (prime, size): the six columns uploaded once, an output of six strided columns"""

    def __init__(self, eng, prime, L):
        self.eng, self.prime, self.L, self.n = eng, prime, L, 1 << L
        p = PRIMES[prime][0]
        self.host = np.concatenate([column(p, L, c) for c in range(BATCH)])
        self.d_in = eng.dev_alloc(BATCH * self.n * 4)
        self.d_out = eng.dev_alloc(BATCH * (self.n + GAP) * 4)
        eng.dev_upload(self.host, self.d_in)

    def free(self):
        self.eng.dev_free(self.d_in)
        self.eng.dev_free(self.d_out)

    def transform(self, leg, column_at=0):
        """-> (batch, n) outputs of one leg (batch 1: of column `column_at`), and the gaps of a strided leg"""
        eng, n, batch = self.eng, self.n, leg["batch"]
        stride = n + GAP if leg["strided"] else n
        d_src = self.d_in + 4 * n * column_at
        if leg["inplace"]:
            eng.dev_upload(self.host, self.d_out)
            d_src = self.d_out
        if leg["strided"]:
            for c in range(batch):
                eng.dev_upload(np.full(GAP, SENTINEL, dtype=np.uint64), self.d_out + 4 * (c * stride + n))
        eng.dev_ntt(d_src, self.d_out, self.L, n_in=n_in_of(leg, n), batch=batch, in_stride=n, out_stride=stride,
                    inverse=leg["inverse"], offset=leg["offset"], post_scale=leg["post"])
        got = eng.dev_download(self.d_out, batch * stride).reshape(batch, stride)
        return got[:, :n], got[:, n:]


def _where(got, want, c):
    bad = np.flatnonzero(np.asarray(got, dtype=np.uint64) != np.asarray(want, dtype=np.uint64))
    if not len(bad):   # the digest differed and the values do not: the manifest is what is wrong
        return {"column": c, "index": None, "differing": 0}
    return {"column": c, "index": int(bad[0]), "differing": int(len(bad))}


def _check_leg(grp, digests, leg, singles):
    """-> (ok, where, kernels): every column against its digest, or -- where the manifest has none -- against the same
    setting's single-column run of the same input"""
    eng = grp.eng
    eng.profile(True)
    try:
        got, gaps = grp.transform(leg)
        kernels = {k: v["launches"] for k, v in eng.profile_read().items() if k.startswith("ntt_")}
    finally:
        eng.profile(False)
    if gaps.size and not (gaps == SENTINEL).all():
        c, i = (int(v[0]) for v in np.nonzero(gaps != SENTINEL))
        return False, {"column": c, "gap_index": i}, kernels
    for c in range(leg["batch"]):
        k = key(grp.prime, grp.L, leg, c)
        if k in digests:
            if digest(got[c]) != digests[k]:
                from oracle import oracle as o
                return False, _where(got[c], oracle_column(o, grp.prime, grp.L, leg, c), c), kernels
        else:
            one = singles(leg, c)
            if not np.array_equal(got[c], one):
                return False, dict(_where(got[c], one, c), against="single-column run"), kernels
    return True, None, kernels


def run(manifest, report=None, families=FAMILIES, plans=None, primes=("ref", "p2")):
    """plans: [(L, plan string)] run as family "custom" on the first of `primes` instead of the table's rows.  -> the report
    (written to `report` as JSON when given): per plan and leg ok, where it first differed, the ntt_* launches recorded;
    the SMI_* variables of this process; seconds."""
    import stark_rs_amd as s
    t0 = time.time()
    with open(manifest) as f:
        digests = json.load(f)["digests"]
    assert not any(k.startswith("SMI_NTT_PLAN_") for k in os.environ)
    if plans:
        todo = [({"id": "custom:%s@%d" % (pl, L), "family": "middle", "L": L, "plan": pl}, primes[0]) for L, pl in plans]
    else:
        todo = entries(families, primes)
    env = {k: v for k, v in os.environ.items() if k.startswith("SMI_")}
    out = {"plans": {}, "env": env, "error": None}
    engines, grp = {}, None
    try:
        for row, prime in todo:
            if prime not in engines:
                engines[prime] = s.Engine(PRIMES[prime][0], PRIMES[prime][1], 0)
            if grp is None or (grp.prime, grp.L) != (prime, row["L"]):
                if grp is not None:
                    grp.free()
                grp = _Group(engines[prime], prime, row["L"])
            t1 = time.time()
            rec = {"L": row["L"], "plan": row["plan"], "family": row["family"], "prime": prime, "legs": {}}
            out["plans"]["%s:%s" % (row["id"], prime)] = rec
            cache = {}

            def singles(leg, c):   # columns 1..4 above 2^20 points: one single-column run per direction, shared by the legs
                k = (leg["inverse"], c)
                if k not in cache:
                    one = dict(leg, batch=1, strided=False, inplace=False)
                    cache[k] = grp.transform(one, column_at=c)[0][0].copy()
                return cache[k]

            name = "SMI_NTT_PLAN_%d" % row["L"]
            os.environ[name] = row["plan"]
            try:
                for leg_name, leg in legs(row["family"], env).items():
                    ok, where, kernels = _check_leg(grp, digests, leg, singles)
                    rec["legs"][leg_name] = {"ok": bool(ok), "where": where, "kernels": kernels}
            finally:
                del os.environ[name]
            rec["seconds"] = round(time.time() - t1, 3)
    except Exception as e:   # a status from the ABI (a HIP error among them) ends the run: nothing further is launched
        out["error"] = "%s: %s" % (type(e).__name__, e)
    else:
        if grp is not None:
            grp.free()
        for e in engines.values():
            e.close()
    out["ok"] = out["error"] is None and all(l["ok"] for r in out["plans"].values() for l in r["legs"].values())
    out["seconds"] = round(time.time() - t0, 2)
    if report:
        with open(report, "w") as f:
            json.dump(out, f, indent=1)
    return out


def main(argv):
    if len(argv) < 3:
        print("usage: ntt_matrix.py MANIFEST.json REPORT.json [--families=a,b] [--plan=L=PLAN ...] [--primes=ref,p2]", file=sys.stderr)
        return 2
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    opt = lambda name: [a[len(name) + 3:] for a in argv[3:] if a.startswith("--%s=" % name)]
    families = tuple(opt("families")[0].split(",")) if opt("families") else FAMILIES
    primes = tuple(opt("primes")[0].split(",")) if opt("primes") else ("ref", "p2")
    plans = [(int(a.split("=", 1)[0]), a.split("=", 1)[1]) for a in opt("plan")]
    out = run(argv[1], argv[2], families, plans, primes)
    for name, rec in out["plans"].items():
        for leg_name, leg in rec["legs"].items():
            if not leg["ok"]:
                print("MISMATCH", name, leg_name, leg["where"])
    if out["error"]:
        print("ERROR", out["error"])
    n_legs = sum(len(r["legs"]) for r in out["plans"].values())
    print("ntt matrix: %d plans, %d legs, %s, %.1f s" % (len(out["plans"]), n_legs, "all equal" if out["ok"] else "FAILED", out["seconds"]))
    return 2 if out["error"] else 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
