"""CPU: the launch plans the HIP launchers execute -- merkle_plan (csrc/merkle_plan.h), fri_layout and fri_round_plan
(csrc/fri_plan.h) -- through the emulator library, which compiles the same headers.  The Merkle plans are compared with
a table recorded from the parent commit's launcher (tests/data/merkle_plans_parent.txt); the round plans are checked
for their invariants over every knob setting, the two that mis-planned before included."""
import ctypes as C
import os

import numpy as np
import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "merkle_plans_parent.txt")
KNOB_NAMES = ["K", "TOP_BLOCKS", "ELEMS_LOG", "SINGLE", "MINCHUNK", "FUSE", "GENERIC"]
DEFAULTS = dict(K=2, TOP_BLOCKS=256, ELEMS_LOG=19, SINGLE=512, MINCHUNK=64, FUSE=1, GENERIC=0)
LEAF, CHUNK, SUB = 0, 1, 2                       # MerkleStep::family
INST_ROWS, INST_K2, INST_GENERIC = 0, 1, 2       # MerkleStep::inst
DIGESTS, ELEMENTS, ROWS = 0, 1, 2                # MerkleShape::leaves
SRC = {0: "N", 1: "C", 2: "Q"}                   # MerkleStep::src_cap
R0_ALIGNED, R0_UNALIGNED, R0_COMBINE = 0, 1, 2
BY_CALLER, BY_FOLD, BY_CHUNK, BY_QUAD, BY_TAIL_HEAD, IN_TAIL = range(6)
TREE_HOOK, TREE_PHASE, TREE_TAIL = range(3)
TAIL_LEN, TAIL_MAX_ROUNDS = 512, 12              # SMI_FRI_TAIL's default, SMI_FRI_TAIL_MAX_ROUNDS


@pytest.fixture(scope="module")
def emu():
    import stark_rs_amd as s
    s.build()
    from stark_rs_amd._lib import EMU_PATH as path
    L = C.CDLL(path)
    i64p, u64p, u8p = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    L.emu_merkle_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, i64p, u64p]
    L.emu_fri_layout.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, u64p, u64p]
    L.emu_fri_layout.restype = None
    L.emu_fri_round_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, i64p, u8p, u8p, C.POINTER(C.c_uint32)]
    return L


def knobs(**over):
    k = dict(DEFAULTS, **over)
    return (C.c_int64 * 7)(*[k[n] for n in KNOB_NAMES])


def merkle_plan(emu, n, n_trees, leaves, row_cols, kn):
    out = (C.c_uint64 * (10 * 64))()
    steps = emu.emu_merkle_plan(n, n_trees, leaves, row_cols, kn, out)
    keys = ["family", "inst", "from_leaves", "level", "count", "arg", "grid", "lds", "ends_root", "src_cap"]
    return [dict(zip(keys, out[10 * i:10 * i + 10])) for i in range(steps)]


def kernel_name(st):
    """the parent's kernel instantiation a step stands for"""
    if st["family"] == LEAF:
        return "leaf"
    if st["family"] == CHUNK:
        return "top<1>" if st["from_leaves"] else "top<0>"
    if st["inst"] == INST_ROWS:
        return "sub<1,0,1>"
    return "sub<%d,%d,0>" % (st["from_leaves"], 2 if st["inst"] == INST_K2 else 0)


def parent_table():
    rows = []
    with open(TABLE) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            parts = [x.strip() for x in line.split("|")]
            kind, logn, trees, knob = parts[0].split()
            steps = [s.split() for s in parts[1].split(";")] if parts[1] else []
            src = dict(kv.split("=") for kv in parts[2].split()) if len(parts) > 2 else None
            rows.append((kind, int(logn), int(trees), knob, steps, src))
    return rows


def test_parent_table_is_complete_and_holds_the_anchors():
    rows = parent_table()
    assert open(TABLE).readline().startswith("# Merkle launch plans of launch_merkle_impl at parent commit 1a3b9a4")
    have = {(k, l, t, kn) for k, l, t, kn, _, _ in rows}
    for kind in ("E", "D", "R4"):
        for trees in (1, 4, 64):
            for logn in range(29):
                assert (kind, logn, trees, "default") in have
    for kn in ("K=1", "K=3", "TOP_BLOCKS=64", "TOP_BLOCKS=1024", "ELEMS_LOG=15", "MINCHUNK=8", "SINGLE=256", "GENERIC=1", "FUSE=0"):
        for logn in range(29):
            assert ("E", logn, 1, kn) in have
    # (kernel, level, count, chunk or K, hook fired) of the anchors: default knobs, element leaves
    brief = {(l, t): [(s[0], int(s[1]), int(s[2]), int(s[3]), int(s[7])) for s in st] for k, l, t, kn, st, _ in rows if k == "E" and kn == "default"}
    assert brief[(9, 1)] == [("top<1>", 0, 512, 512, 1)]
    assert brief[(12, 1)] == [("top<1>", 0, 4096, 64, 0), ("top<0>", 6, 64, 64, 1)]
    assert brief[(19, 1)] == [("top<1>", 0, 1 << 19, 2048, 0), ("top<0>", 11, 256, 256, 1)]
    assert brief[(20, 1)] == [("sub<1,2,0>", 0, 1 << 20, 2, 0), ("top<0>", 2, 1 << 18, 1024, 0), ("top<0>", 12, 256, 256, 1)]
    assert brief[(25, 1)] == [("sub<1,2,0>", 0, 1 << 25, 2, 0), ("sub<0,2,0>", 2, 1 << 23, 2, 0), ("sub<0,2,0>", 4, 1 << 21, 2, 0),
                              ("top<0>", 6, 1 << 19, 2048, 0), ("top<0>", 17, 256, 256, 1)]
    assert brief[(25, 4)] == [("sub<1,2,0>", 0, 1 << 25, 2, 0), ("sub<0,2,0>", 2, 1 << 23, 2, 0), ("sub<0,2,0>", 4, 1 << 21, 2, 0),
                              ("sub<0,2,0>", 6, 1 << 19, 2, 0), ("top<0>", 8, 1 << 17, 2048, 0), ("top<0>", 19, 64, 64, 0)]


def test_merkle_plan_reproduces_every_plan_of_the_parent(emu):
    checked = 0
    for kind, logn, trees, knob, want, src in parent_table():
        kn = knobs() if knob == "default" else knobs(**{knob.split("=")[0]: int(knob.split("=")[1])})
        leaves, row_cols = {"E": (ELEMENTS, 0), "D": (DIGESTS, 0), "R4": (ROWS, 4)}[kind]
        plan = merkle_plan(emu, 1 << logn, trees, leaves, row_cols, kn)
        got = []
        for st in plan:
            threads = 1024 if st["family"] == CHUNK else 256
            row = [kernel_name(st), st["level"], st["count"], st["arg"], st["grid"], threads, st["lds"], st["ends_root"]]
            got += [[str(x) for x in row]] * (trees if st["family"] == LEAF else 1)   # a lone leaf: one launch per tree
        assert got == want, (kind, logn, trees, knob)
        if src is not None:
            cap = SRC[plan[0]["src_cap"]] if plan else "N"
            assert cap == src["promised"], (logn, knob)
            # what the parent's callers relied on is what its first launch did with a source (FUSE=0 only switches it off)
            if cap != "N":
                assert src["fold"] == cap and src["combine"] == ("Q" if cap == "Q" else "N"), (logn, knob)
        assert all(st["src_cap"] == 0 for st in plan[1:])
        checked += 1
    assert checked == 3 * 3 * 29 + 9 * 29


# ------------------------------------------------------------------------- FRI
def ref_rounds(n, expansion, t):
    """Fri::num_rounds, src/fri.rs:93-103"""
    r = 0
    while n > expansion and 4 * t < n:
        n //= 2
        r += 1
    return r


def fri_configs():
    """(log len, expansion, t, R) with R >= 1 and t <= the last codeword's length (src/fri.rs:183-192)"""
    out = []
    for loglen in range(3, 31):
        for expansion in (4, 8):
            for t in (1, 8, 32):
                R = ref_rounds(1 << loglen, expansion, t)
                if R >= 1 and t <= (1 << loglen) >> (R - 1):
                    out.append((loglen, expansion, t, R))
    return out


KNOB_SETTINGS = [{}, dict(K=1), dict(K=3), dict(TOP_BLOCKS=64), dict(TOP_BLOCKS=1024), dict(ELEMS_LOG=15), dict(MINCHUNK=8), dict(SINGLE=256),
                 dict(GENERIC=1), dict(FUSE=0),
                 dict(SINGLE=4096), dict(MINCHUNK=4096), dict(K=3, SINGLE=4096)]   # the last three mis-planned before


def round_plan(emu, n, R, phase, round0, kn, tail_len=TAIL_LEN):
    prod, tree, tail_at = (C.c_uint8 * 64)(), (C.c_uint8 * 64)(), C.c_uint32()
    ok = emu.emu_fri_round_plan(n, R, phase, tail_len, round0, kn, prod, tree, C.byref(tail_at))
    return bool(ok), list(prod[:R]), list(tree[:R]), tail_at.value


def parent_fuse_combine(n, k):
    """merkle_fuses_leaf_source(n) && n > fri_tail_len() of the parent (stark.hip's fuse_combine, fri_run's check)"""
    k = dict(DEFAULTS, **k)
    elems_max = min(1 << k["ELEMS_LOG"], 2048 * k["TOP_BLOCKS"])
    off = k["FUSE"] == 0 or k["GENERIC"] != 0 or k["K"] != 2
    return (not off) and n >= 8 and n > elems_max and n > TAIL_LEN


def test_round_plan_invariants_over_every_knob_setting(emu):
    cfgs = fri_configs()
    have = {(l, e, t) for l, e, t, _ in cfgs}
    for loglen in range(8, 31):
        for expansion in (4, 8):
            for t in (1, 8, 32):
                assert (loglen, expansion, t) in have
    for over in KNOB_SETTINGS:
        kn = knobs(**over)
        cap = {}   # what the first step of a single tree of 2^l elements can do with computed leaves
        for l in range(0, 31):
            plan = merkle_plan(emu, 1 << l, 1, ELEMENTS, 0, kn)
            cap[l] = plan[0]["src_cap"]
        fuse = dict(DEFAULTS, **over)["FUSE"] != 0
        for loglen, expansion, t, R in cfgs:
            n = 1 << loglen
            for phase in (0, 5):
                for round0 in (R0_ALIGNED, R0_UNALIGNED, R0_COMBINE):
                    ok, prod, tree, tail_at = round_plan(emu, n, R, phase, round0, kn)
                    where = (over, loglen, expansion, t, phase, round0)
                    if round0 == R0_COMBINE:
                        assert ok == parent_fuse_combine(n, over), where   # otherwise fri_run answers BAD_ARG, as before
                        if not ok:
                            continue
                        assert cap[loglen] == 2, where
                    assert ok, where
                    # every codeword has exactly one producer (one entry per round, of the kinds its place allows)
                    assert len(prod) == R and len(tree) == R
                    assert prod[0] == (BY_QUAD if round0 == R0_COMBINE else BY_CALLER), where
                    assert all(p in (BY_FOLD, BY_CHUNK, BY_QUAD, BY_TAIL_HEAD, IN_TAIL) for p in prod[1:]), where
                    for r in range(1, R):
                        if prod[r] == BY_CHUNK:
                            assert cap[loglen - r] == 1, where
                        if prod[r] == BY_QUAD:
                            assert cap[loglen - r] == 2, where
                            assert r > 1 or round0 != R0_UNALIGNED, where   # only between aligned buffers
                        if prod[r] in (BY_CHUNK, BY_QUAD, BY_TAIL_HEAD):
                            assert fuse, where
                    # the tail: only at phase 0, from a codeword of at most tail_len elements, at most 12 rounds
                    assert tail_at <= R
                    if tail_at < R:
                        assert phase == 0 and (n >> tail_at) <= TAIL_LEN and R - tail_at <= TAIL_MAX_ROUNDS, where
                    for r in range(R):
                        assert tree[r] == (TREE_TAIL if r >= tail_at else (TREE_PHASE if phase else TREE_HOOK)), where
                        # a fold elided into the tail only when the tail runs, and the tail's own folds nowhere else
                        if r:
                            assert (prod[r] == IN_TAIL) == (r > tail_at), where
                            if prod[r] == BY_TAIL_HEAD:
                                assert r == tail_at, where
                    # the rounds sum to R
                    assert sum(1 for x in tree if x != TREE_TAIL) + (R - tail_at) == R, where


def test_round_plan_of_the_documented_prove(emu):
    """2^21 elements, expansion 8, 8 tests, phase 0, default knobs (the docstring of
    test_fri_prove_with_folds_computed_by_the_leaf_kernel_is_byte_identical): 16 rounds"""
    R = ref_rounds(1 << 21, 8, 8)
    assert R == 16
    for round0, first_fold in ((R0_ALIGNED, BY_QUAD), (R0_UNALIGNED, BY_FOLD)):
        ok, prod, tree, tail_at = round_plan(emu, 1 << 21, R, 0, round0, knobs())
        assert ok
        assert prod == [BY_CALLER, first_fold] + [BY_CHUNK] * 10 + [BY_TAIL_HEAD] + [IN_TAIL] * 3   # 2^19 .. 2^10, then 2^9 at the tail's head
        assert tree == [TREE_HOOK] * 12 + [TREE_TAIL] * 4 and tail_at == 12


def test_knobs_that_mis_planned_before_fall_back_to_what_the_first_launch_takes(emu):
    # SINGLE=4096: the 4096-element tree starts with the four-leaves-per-lane kernel, not with the chunk kernel it was promised to
    R = ref_rounds(1 << 14, 8, 8)
    _, prod, _, _ = round_plan(emu, 1 << 14, R, 5, R0_ALIGNED, knobs(SINGLE=4096))
    assert prod[2] == BY_QUAD and prod[1] == BY_CHUNK
    # with K=3 that kernel cannot compute leaves at all: a fold launch, where the parent answered BAD_ARG in mid-prove
    _, prod, _, _ = round_plan(emu, 1 << 14, R, 5, R0_ALIGNED, knobs(K=3, SINGLE=4096))
    assert prod[2] == BY_FOLD and prod[1] == BY_CHUNK


def test_fri_layout_against_the_oracle(emu, oracle):
    o = oracle
    for loglen, expansion, t in ((6, 4, 2), (8, 8, 8), (10, 4, 1), (7, 8, 4), (9, 4, 16)):
        N = 1 << loglen
        cfg = o.fri_cfg(o.ff_prim_nth_root(N), 3, N, expansion, t)
        proof, _ = o.fri_prove(cfg, o.splitmix64(loglen, N) % np.uint64(o.P_REF))
        head, offs = (C.c_uint64 * 5)(), (C.c_uint64 * 128)()
        emu.emu_fri_layout(N, expansion, t, 1, head, offs)
        R, last_n, off_last, off_layers, proof_len = list(head)
        assert R == o.fri_num_rounds(cfg) == ref_rounds(N, expansion, t)
        assert last_n == N >> (R - 1) and off_last == 33 * R and off_layers == off_last + 9 + 8 * last_n
        assert proof_len == len(proof)
        # tags of the serialized stream at the offsets the layout names (src/stream.rs:39-60): 2 = FieldElements, 3 = MerklePath
        assert proof[off_last] == 2
        for i in range(R - 1):
            assert proof[offs[2 * i]] == 2 and proof[offs[2 * i + 1]] == 3
        emu.emu_fri_layout(N, expansion, t, 0, head, offs)
        assert head[4] == off_layers


# ------------------------------------------------------- what the GPU battery (tests/gpu_battery.py) must reach
def step_signature(st, kind):
    """what tells one launch of launch_merkle_impl from another: the kernel family and instantiation, where level 0 comes
    from (the leaf kind, when this step hashes leaves), K or the chunk size, whether it ends with the root, and what it
    can do with computed leaves"""
    return (st["family"], st["inst"], kind if st["from_leaves"] else "-", st["arg"], st["ends_root"], st["src_cap"])


def test_battery_trees_take_every_step_a_single_tree_takes(emu):
    """A coverage condition, not a measurement: under each of the thirteen knob settings, every step signature that a
    single tree of up to 2^23 leaves takes -- element, digest or row leaves -- is taken by some tree of the battery that
    tests/test_gpu_plans.py runs on the GPU under that setting.  The battery's trees stop at 2^21 leaves; only under
    TOP_BLOCKS=1024 do steps first appear above that, and for that setting alone its two extra trees count."""
    import gpu_battery as gb
    shape = {"E": (ELEMENTS, 0), "D": (DIGESTS, 0), "R": (ROWS, 4)}

    def battery_plan(kind, logn, w, kn):
        if kind == "R" and w > 4:      # launch_merkle_rows: rows wider than four columns are hashed first, then a tree of digests
            return "D", merkle_plan(emu, 1 << logn, 1, DIGESTS, 0, kn)
        leaves, cols = shape[kind]
        return kind, merkle_plan(emu, 1 << logn, 1, leaves, w if kind == "R" else cols, kn)

    assert set(gb.EXTRA_TREES) == {"Dx22", "Rx22"}
    for over in KNOB_SETTINGS:
        kn = knobs(**over)
        have = set()
        for name, (kind, logn, w, _full) in gb.tree_items(extras=over == dict(TOP_BLOCKS=1024)).items():
            k, plan = battery_plan(kind, logn, w, kn)
            have |= {step_signature(st, k) for st in plan}
        for kind, (leaves, cols) in shape.items():
            for logn in range(24):
                for st in merkle_plan(emu, 1 << logn, 1, leaves, cols, kn):
                    assert step_signature(st, kind) in have, (over, kind, logn, st)
    # the extras are the smallest trees that take the two late steps of TOP_BLOCKS=1024, and they are needed
    kn = knobs(TOP_BLOCKS=1024)
    late = {"D": (SUB, INST_K2, "-", 2, 0, 0), "R": (SUB, INST_ROWS, "R", 2, 0, 0)}
    for kind, sig in late.items():
        leaves, cols = shape[kind]
        first = min(l for l in range(24) if sig in {step_signature(st, kind) for st in merkle_plan(emu, 1 << l, 1, leaves, cols, kn)})
        assert first == 22 and gb.EXTRA_TREES[kind + "x22"][1] == 22
        for other in ("E", "D", "R"):
            lv, cc = shape[other]
            for l in range(22):
                assert sig not in {step_signature(st, other) for st in merkle_plan(emu, 1 << l, 1, lv, cc, kn)}
