"""The argument checks of the nine inter TU entries, pinned by table: every invalid-argument case a launcher checks, driven through the
C entry, and the pair (return code, x265hip_last_error() text) compared against literals.  The literals (EXPECT, at the end of this file)
were recorded when each of the four launchers still carried its own copy of the checks; every recorded code was X265HIP_EINVAL.  What is
asserted: a record is refused with the same code and the same words, and the same checks still run before the device is asked for.

Before every call an invalid x265hip_tu_launch_grid call leaves SENTINEL as the error text: a call that returns without setting a text of
its own - a valid record, or X265HIP_ENODEV from an entry whose check waits behind the device - leaves SENTINEL there.

CPU part: the cases reachable without a device, everywhere; where no device is present also the others and valid records of every
entry, which give X265HIP_ENODEV.  GPU part: every invalid case with its operands in device memory - each returns before anything is
launched - and the valid calls of x265hip_tu_launch_grid, which return a grid and launch nothing."""
import ctypes
import importlib

import pytest
import torch

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")

EINVAL, ENODEV = -2, -1
SENTINEL = "tu_launch_grid: entry 7"
OPERANDS = ("fenc", "fref", "recon", "mv", "levels", "num_sig", "dist", "fref1", "mv1", "ref_idx", "qp_map", "plane0", "plane1", "plane2", "plane3")
TABLES = A.TuTablesRec()          # a host record of NULL device pointers: no invalid case gets as far as reading it

# entry -> (record kind, records per call)
ENTRIES = {
    "x265hip_inter_recon": ("uni", 1), "x265hip_inter_recon_chroma": ("uni", 1), "x265hip_inter_recon_chroma_pair": ("uni", 2),
    "x265hip_inter_recon_bi": ("bi", 1), "x265hip_inter_recon_chroma_bi": ("bi", 1),
    "x265hip_inter_recon_refs": ("refs", 1), "x265hip_inter_recon_chroma_refs": ("refs", 1), "x265hip_inter_recon_chroma_pair_refs": ("refs", 2),
    "x265hip_tu_launch_grid": ("grid", 0),
}
RECORD = {"uni": S.ReconParams, "bi": S.ReconBiParams, "refs": A.ReconRefsParams}
OWN = {"uni": (), "bi": ("fref1", "mv1"), "refs": ("nrefs", "ref_idx")}          # the fields that are not the base record's


def host_operands():
    """Placeholders: without a device no entry gets as far as using them, and no check dereferences an operand."""
    return {k: 0x100000 * (i + 1) for i, k in enumerate(OPERANDS)}


def device_operands():
    """One zeroed MiB of device memory per operand, the pointer in its middle."""
    keep = [torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0") for _ in OPERANDS]
    ops = {k: t.data_ptr() + (1 << 19) for k, t in zip(OPERANDS, keep)}
    ops["keep"] = keep
    return ops


def record(kind, ops, spec, keep):
    """A valid 128 x 64 8-bit record of 32 x 32 luma blocks (four reference planes where it takes a table of them), then `spec` applied:
    field -> value; tables / qp_map -> whether the record has one; planes -> {k: fref[k]}; weight0 / weight1 -> (present, weight, offset,
    log2_denom).  spec None = a NULL record."""
    if spec is None:
        return None
    r = RECORD[kind]()
    p = r if kind == "uni" else r.base
    p.depth, p.width, p.height, p.level, p.qp = 8, 128, 64, 2, 30
    p.fenc, p.fenc_stride, p.fref, p.fref_stride, p.recon, p.recon_stride = ops["fenc"], 320, ops["fref"], 320, ops["recon"], 320
    p.mv, p.levels, p.num_sig, p.dist = ops["mv"], ops["levels"], ops["num_sig"], ops["dist"]
    if kind == "bi":
        r.fref1, r.mv1 = ops["fref1"], ops["mv1"]
    if kind == "refs":
        r.nrefs, r.ref_idx = 4, ops["ref_idx"]
        for k in range(4):
            r.fref[k] = ops[f"plane{k}"]
    for k, v in spec.items():
        if k == "tables":
            p.tables = ctypes.addressof(TABLES) if v else None
        elif k == "qp_map":
            p.qp_map = ops["qp_map"] if v else None
        elif k == "planes":
            for i, plane in v.items():
                r.fref[i] = plane
        elif k in ("weight0", "weight1"):
            keep.append(S.PredWeight(*v))
            setattr(r, k, ctypes.pointer(keep[-1]))
        else:
            setattr(r if k in OWN[kind] else p, k, v)
    return r


def call(L, entry, ops, specs):
    """(return code, error text) of one call; SENTINEL is the text in front of it."""
    grid = L.x265hip_tu_launch_grid
    grid.argtypes = [ctypes.c_int] * 6
    assert grid(7, 16, 8, 0, 1, 100) == EINVAL and L.x265hip_last_error().decode() == SENTINEL
    kind, nrec = ENTRIES[entry]
    if kind == "grid":
        rc = grid(*specs)
    else:
        keep = []
        recs = [record(kind, ops, s, keep) for s in specs]
        f = getattr(L, entry)
        f.argtypes = [ctypes.POINTER(RECORD[kind])] * nrec + [ctypes.c_void_p]
        rc = f(*[ctypes.byref(r) if r is not None else None for r in recs], None)
    return rc, L.x265hip_last_error().decode()


# the cases of one record: (id, spec)
NULLS = [(f"{k}=NULL", {k: None}) for k in ("fenc", "fref", "recon", "mv", "levels", "num_sig", "dist")]
BASE = [("width=100", {"width": 100}), ("height=-64", {"height": -64}), ("depth=9", {"depth": 9}), ("level=-1", {"level": -1}), ("level=3", {"level": 3}),
        ("qp=-1", {"qp": -1}), ("depth=10,qp=64", {"depth": 10, "qp": 64})]
MAP_AND_TABLES = ("qp_map+tables", {"qp_map": True, "tables": True})
NULL_RECORD = ("NULL record", None)
WEIGHTS = [("weight0:log2_denom=8", {"weight0": (1, 64, 0, 8)}), ("weight0:weight=-129", {"weight0": (0, -129, 0, 6)}),
           ("weight0:offset=128", {"weight0": (1, 64, 128, 6)}), ("weight1:log2_denom=-1", {"weight1": (1, 64, 0, -1)})]
# the multi-reference launcher: tables first, then the operands, nrefs, the planes of the table, the base record - the three combined cases pin that order
REFS_ORDER = [("nrefs=0,width=100", {"nrefs": 0, "width": 100}), ("fenc=NULL,nrefs=0", {"fenc": None, "nrefs": 0}), ("tables,fenc=NULL", {"tables": True, "fenc": None})]
REFS = ([("tables", {"tables": True})] + [c for c in NULLS if c[0] != "fref=NULL"] + [("ref_idx=NULL", {"ref_idx": None}), ("nrefs=0", {"nrefs": 0}), ("nrefs=9", {"nrefs": 9}),
        ("plane0=NULL", {"planes": {0: None}}), ("plane3=NULL", {"planes": {3: None}})] + REFS_ORDER + BASE)
REFS_PAIR = ([("tables", {"tables": True}), NULLS[0], ("ref_idx=NULL", {"ref_idx": None}), ("nrefs=9", {"nrefs": 9}), ("plane3=NULL", {"planes": {3: None}})] +
             REFS_ORDER + BASE)
VALID_REFS = [("valid", {}), ("base.fref=NULL", {"fref": None}), ("nrefs=2,plane3=NULL", {"nrefs": 2, "planes": {3: None}}), ("qp_map", {"qp_map": True})]
BI = [MAP_AND_TABLES, NULL_RECORD] + NULLS + [("fref1=NULL", {"fref1": None}), ("mv1=NULL", {"mv1": None})] + BASE + WEIGHTS


def pair(cases, extra):
    """The cases of a two-record entry: every case of one record in the first (cb) and in the second (cr), the other valid; then `extra`."""
    return [("cb:" + i, (s, {})) for i, s in cases] + [("cr:" + i, ({}, s)) for i, s in cases] + extra


NULL_RECORDS = [("cb:NULL record", (None, {})), ("cr:NULL record", ({}, None)), ("both:NULL record", (None, None))]
PLANES_DIFFER = [("cr:level=1", ({}, {"level": 1})), ("cr:width=64", ({}, {"width": 64})), ("cr:height=128", ({}, {"height": 128})), ("cr:depth=10", ({}, {"depth": 10}))]
EARLY = ("qp_map+tables", "NULL record")          # what the uni-predictive chroma entries check before the device (x265hip_inter_recon and the bi-predictive ones: the first alone)

# entry -> [(id, the record specs of the call, checked before the device is asked for)]
CASES = {
    "x265hip_inter_recon": [(i, (s,), i == EARLY[0]) for i, s in [MAP_AND_TABLES, NULL_RECORD] + NULLS + BASE],
    "x265hip_inter_recon_chroma": [(i, (s,), i in EARLY) for i, s in [MAP_AND_TABLES, NULL_RECORD] + NULLS + BASE],
    "x265hip_inter_recon_chroma_pair": [(i, s, i[3:] in EARLY or i == "both:NULL record") for i, s in pair(
        [MAP_AND_TABLES, NULLS[0], NULLS[-1]] + BASE,
        NULL_RECORDS + PLANES_DIFFER + [("cr:tables", ({}, {"tables": True})), ("cb:tables", ({"tables": True}, {}))])],
    "x265hip_inter_recon_bi": [(i, (s,), i == EARLY[0]) for i, s in BI],
    "x265hip_inter_recon_chroma_bi": [(i, (s,), i == EARLY[0]) for i, s in BI],
    "x265hip_inter_recon_refs": [(i, (s,), True) for i, s in [NULL_RECORD] + REFS],
    "x265hip_inter_recon_chroma_refs": [(i, (s,), True) for i, s in [NULL_RECORD] + REFS],
    "x265hip_inter_recon_chroma_pair_refs": [(i, s, True) for i, s in pair(REFS_PAIR, NULL_RECORDS + PLANES_DIFFER + [("cr:nrefs=3", ({}, {"nrefs": 3}))])],
    "x265hip_tu_launch_grid": [("%d,%d,%d,%d,%d,%d" % a, a, True) for a in (
        (-1, 16, 8, 0, 1, 100), (5, 16, 8, 0, 1, 100), (7, 16, 8, 0, 1, 100), (10, 16, 8, 0, 1, 100),
        (0, 4, 8, 0, 1, 100), (0, 64, 8, 0, 1, 100), (1, 4, 8, 0, 1, 100), (2, 32, 8, 0, 1, 100), (3, 32, 8, 0, 1, 100), (4, 2, 8, 0, 1, 100),
        (8, 4, 8, 0, 1, 100), (9, 32, 8, 0, 1, 100), (0, 16, 9, 0, 1, 100), (0, 16, 16, 0, 1, 100), (8, 16, 8, 1, 1, 100), (9, 16, 8, 1, 2, 100),
        (0, 16, 8, 0, 2, 100), (1, 16, 8, 0, 2, 100), (3, 16, 8, 0, 2, 100), (4, 16, 8, 0, 2, 100), (8, 16, 8, 0, 2, 100), (2, 16, 8, 0, 3, 100),
        (9, 16, 8, 0, 0, 100), (0, 16, 8, 0, 1, 0), (2, 16, 8, 1, 2, -5))],
}

# valid calls: (id, specs).  The eight launching entries get them only where no device is present.
VALID = {
    "x265hip_inter_recon": [("valid", ({},)), ("tables", ({"tables": True},)), ("qp_map", ({"qp_map": True},))],
    "x265hip_inter_recon_chroma": [("valid", ({},)), ("tables", ({"tables": True},))],
    "x265hip_inter_recon_chroma_pair": [("valid", ({}, {})), ("tables", ({"tables": True}, {"tables": True}))],
    "x265hip_inter_recon_bi": [("valid", ({},)), ("weights", ({"weight0": (1, 64, 0, 6), "weight1": (1, -128, 127, 7)},))],
    "x265hip_inter_recon_chroma_bi": [("valid", ({},)), ("tables", ({"tables": True},))],
    "x265hip_inter_recon_refs": [(i, (s,)) for i, s in VALID_REFS],
    "x265hip_inter_recon_chroma_refs": [(i, (s,)) for i, s in VALID_REFS],
    "x265hip_inter_recon_chroma_pair_refs": [(i, (s, s)) for i, s in VALID_REFS],
    # five blocks: fewer than one resident set of any persistent kernel, so the grid is the number of blocks at every size
    "x265hip_tu_launch_grid": [("%d,%d,%d,%d,%d,%d" % a, a) for a in (
        (0, 8, 8, 0, 1, 5), (0, 16, 10, 1, 1, 5), (0, 32, 12, 0, 1, 5), (1, 8, 8, 1, 1, 5), (1, 32, 10, 0, 1, 5), (2, 4, 8, 0, 2, 5), (2, 16, 10, 1, 2, 5),
        (3, 8, 8, 0, 1, 5), (3, 16, 12, 1, 1, 5), (4, 4, 8, 0, 1, 5), (4, 32, 10, 1, 1, 5), (8, 8, 8, 0, 1, 5), (8, 32, 10, 0, 1, 5), (9, 4, 8, 0, 2, 5),
        (9, 16, 10, 0, 2, 5))],
}
VALID_GRID = 5


def prime(L):
    """The first call that asks for the device, so that its one-time initialisation (which may set a text) lies behind every case."""
    f = L.x265hip_tu_launch_grid
    f.argtypes = [ctypes.c_int] * 6
    f(0, 16, 8, 0, 1, 1)


def test_every_case_has_its_literal():
    for entry in ENTRIES:
        ids = [c[0] for c in CASES[entry]]
        assert len(set(ids)) == len(ids) and set(ids) == set(EXPECT[entry]), (entry, set(ids) ^ set(EXPECT[entry]))
    assert set(EXPECT) == set(ENTRIES) == set(VALID)


@pytest.mark.parametrize("entry", ENTRIES)
def test_checks_in_front_of_the_device(entry):
    L = A.lib()
    prime(L)
    no_device = not torch.cuda.is_available()
    ops = host_operands()
    for cid, specs, early in CASES[entry]:
        if early:
            assert call(L, entry, ops, specs) == (EINVAL, EXPECT[entry][cid]), cid
        elif no_device:
            assert call(L, entry, ops, specs) == (ENODEV, SENTINEL), cid          # the check waits behind the device
    if no_device:
        for cid, specs in VALID[entry]:
            assert call(L, entry, ops, specs) == (ENODEV, SENTINEL), cid


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_checks_with_a_device(entry):
    L = A.lib()
    prime(L)
    ops = device_operands()
    for cid, specs, _ in CASES[entry]:
        assert call(L, entry, ops, specs) == (EINVAL, EXPECT[entry][cid]), cid
    if entry == "x265hip_tu_launch_grid":
        for cid, specs in VALID[entry]:
            assert call(L, entry, ops, specs) == (VALID_GRID, SENTINEL), cid


_MAP = "qp_map together with tables (scaling-list tables are selected per qp % 6)"
_NO_TABLES = "tables (scaling lists / the denoiser) are not supported by this stage"
_DIFFER = "the two planes differ in geometry / depth / level / "

EXPECT = {
    "x265hip_inter_recon": {
        "qp_map+tables": "inter_recon: " + _MAP,
        "NULL record": "inter_recon: NULL operand",
        "fenc=NULL": "inter_recon: NULL operand",
        "fref=NULL": "inter_recon: NULL operand",
        "recon=NULL": "inter_recon: NULL operand",
        "mv=NULL": "inter_recon: NULL operand",
        "levels=NULL": "inter_recon: NULL operand",
        "num_sig=NULL": "inter_recon: NULL operand",
        "dist=NULL": "inter_recon: NULL operand",
        "width=100": "inter_recon: width/height must be multiples of 64",
        "height=-64": "inter_recon: width/height must be multiples of 64",
        "depth=9": "inter_recon: depth 9",
        "level=-1": "inter_recon: level -1 (0..2 = 8x8, 16x16, 32x32)",
        "level=3": "inter_recon: level 3 (0..2 = 8x8, 16x16, 32x32)",
        "qp=-1": "inter_recon: qp -1 out of range",
        "depth=10,qp=64": "inter_recon: qp 64 out of range",
    },
    "x265hip_inter_recon_chroma": {
        "qp_map+tables": "inter_recon_chroma: " + _MAP,
        "NULL record": "inter_recon_chroma: NULL operand",
        "fenc=NULL": "inter_recon_chroma: NULL operand",
        "fref=NULL": "inter_recon_chroma: NULL operand",
        "recon=NULL": "inter_recon_chroma: NULL operand",
        "mv=NULL": "inter_recon_chroma: NULL operand",
        "levels=NULL": "inter_recon_chroma: NULL operand",
        "num_sig=NULL": "inter_recon_chroma: NULL operand",
        "dist=NULL": "inter_recon_chroma: NULL operand",
        "width=100": "inter_recon_chroma: width/height (luma) must be multiples of 64",
        "height=-64": "inter_recon_chroma: width/height (luma) must be multiples of 64",
        "depth=9": "inter_recon_chroma: depth 9",
        "level=-1": "inter_recon_chroma: level -1 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "level=3": "inter_recon_chroma: level 3 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "qp=-1": "inter_recon_chroma: qp -1 out of range",
        "depth=10,qp=64": "inter_recon_chroma: qp 64 out of range",
    },
    "x265hip_inter_recon_chroma_pair": {
        "cb:qp_map+tables": "inter_recon_chroma: " + _MAP,
        "cb:fenc=NULL": "inter_recon_chroma: NULL operand",
        "cb:dist=NULL": "inter_recon_chroma: NULL operand",
        "cb:width=100": "inter_recon_chroma: width/height (luma) must be multiples of 64",
        "cb:height=-64": "inter_recon_chroma: width/height (luma) must be multiples of 64",
        "cb:depth=9": "inter_recon_chroma: depth 9",
        "cb:level=-1": "inter_recon_chroma: level -1 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "cb:level=3": "inter_recon_chroma: level 3 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "cb:qp=-1": "inter_recon_chroma: qp -1 out of range",
        "cb:depth=10,qp=64": "inter_recon_chroma: qp 64 out of range",
        "cr:qp_map+tables": "inter_recon_chroma: " + _MAP,
        "cr:fenc=NULL": "inter_recon_chroma: NULL operand",
        "cr:dist=NULL": "inter_recon_chroma: NULL operand",
        "cr:width=100": "inter_recon_chroma: width/height (luma) must be multiples of 64",
        "cr:height=-64": "inter_recon_chroma: width/height (luma) must be multiples of 64",
        "cr:depth=9": "inter_recon_chroma: depth 9",
        "cr:level=-1": "inter_recon_chroma: level -1 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "cr:level=3": "inter_recon_chroma: level 3 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "cr:qp=-1": "inter_recon_chroma: qp -1 out of range",
        "cr:depth=10,qp=64": "inter_recon_chroma: qp 64 out of range",
        "cb:NULL record": "inter_recon_chroma_pair: NULL operand",
        "cr:NULL record": "inter_recon_chroma_pair: NULL operand",
        "both:NULL record": "inter_recon_chroma_pair: NULL operand",
        "cr:level=1": "inter_recon_chroma: " + _DIFFER + "use of tables",
        "cr:width=64": "inter_recon_chroma: " + _DIFFER + "use of tables",
        "cr:height=128": "inter_recon_chroma: " + _DIFFER + "use of tables",
        "cr:depth=10": "inter_recon_chroma: " + _DIFFER + "use of tables",
        "cr:tables": "inter_recon_chroma: " + _DIFFER + "use of tables",
        "cb:tables": "inter_recon_chroma: " + _DIFFER + "use of tables",
    },
    "x265hip_inter_recon_bi": {
        "qp_map+tables": "inter_recon_bi: " + _MAP,
        "NULL record": "inter_recon_bi: NULL operand",
        "fenc=NULL": "inter_recon_bi: NULL operand",
        "fref=NULL": "inter_recon_bi: NULL operand",
        "recon=NULL": "inter_recon_bi: NULL operand",
        "mv=NULL": "inter_recon_bi: NULL operand",
        "levels=NULL": "inter_recon_bi: NULL operand",
        "num_sig=NULL": "inter_recon_bi: NULL operand",
        "dist=NULL": "inter_recon_bi: NULL operand",
        "fref1=NULL": "inter_recon_bi: NULL operand",
        "mv1=NULL": "inter_recon_bi: NULL operand",
        "width=100": "inter_recon_bi: width/height must be multiples of 64",
        "height=-64": "inter_recon_bi: width/height must be multiples of 64",
        "depth=9": "inter_recon_bi: depth 9",
        "level=-1": "inter_recon_bi: level -1 (0..2 = 8x8, 16x16, 32x32)",
        "level=3": "inter_recon_bi: level 3 (0..2 = 8x8, 16x16, 32x32)",
        "qp=-1": "inter_recon_bi: qp -1 out of range",
        "depth=10,qp=64": "inter_recon_bi: qp 64 out of range",
        "weight0:log2_denom=8": "inter_recon_bi: weight 64 / offset 0 / log2_denom 8 of list 0 out of range",
        "weight0:weight=-129": "inter_recon_bi: weight -129 / offset 0 / log2_denom 6 of list 0 out of range",
        "weight0:offset=128": "inter_recon_bi: weight 64 / offset 128 / log2_denom 6 of list 0 out of range",
        "weight1:log2_denom=-1": "inter_recon_bi: weight 64 / offset 0 / log2_denom -1 of list 1 out of range",
    },
    "x265hip_inter_recon_refs": {
        "NULL record": "inter_recon_refs: NULL operand",
        "tables": "inter_recon_refs: " + _NO_TABLES,
        "fenc=NULL": "inter_recon_refs: NULL operand",
        "recon=NULL": "inter_recon_refs: NULL operand",
        "mv=NULL": "inter_recon_refs: NULL operand",
        "levels=NULL": "inter_recon_refs: NULL operand",
        "num_sig=NULL": "inter_recon_refs: NULL operand",
        "dist=NULL": "inter_recon_refs: NULL operand",
        "ref_idx=NULL": "inter_recon_refs: NULL operand",
        "nrefs=0": "inter_recon_refs: nrefs 0 out of [1,8]",
        "nrefs=9": "inter_recon_refs: nrefs 9 out of [1,8]",
        "plane0=NULL": "inter_recon_refs: NULL plane of reference 0",
        "plane3=NULL": "inter_recon_refs: NULL plane of reference 3",
        "nrefs=0,width=100": "inter_recon_refs: nrefs 0 out of [1,8]",
        "fenc=NULL,nrefs=0": "inter_recon_refs: NULL operand",
        "tables,fenc=NULL": "inter_recon_refs: " + _NO_TABLES,
        "width=100": "inter_recon_refs: width/height (luma) must be multiples of 64",
        "height=-64": "inter_recon_refs: width/height (luma) must be multiples of 64",
        "depth=9": "inter_recon_refs: depth 9",
        "level=-1": "inter_recon_refs: level -1 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "level=3": "inter_recon_refs: level 3 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "qp=-1": "inter_recon_refs: qp -1 out of range",
        "depth=10,qp=64": "inter_recon_refs: qp 64 out of range",
    },
    "x265hip_inter_recon_chroma_refs": {
        "NULL record": "inter_recon_chroma_refs: NULL operand",
        "tables": "inter_recon_chroma_refs: " + _NO_TABLES,
        "fenc=NULL": "inter_recon_chroma_refs: NULL operand",
        "recon=NULL": "inter_recon_chroma_refs: NULL operand",
        "mv=NULL": "inter_recon_chroma_refs: NULL operand",
        "levels=NULL": "inter_recon_chroma_refs: NULL operand",
        "num_sig=NULL": "inter_recon_chroma_refs: NULL operand",
        "dist=NULL": "inter_recon_chroma_refs: NULL operand",
        "ref_idx=NULL": "inter_recon_chroma_refs: NULL operand",
        "nrefs=0": "inter_recon_chroma_refs: nrefs 0 out of [1,8]",
        "nrefs=9": "inter_recon_chroma_refs: nrefs 9 out of [1,8]",
        "plane0=NULL": "inter_recon_chroma_refs: NULL plane of reference 0",
        "plane3=NULL": "inter_recon_chroma_refs: NULL plane of reference 3",
        "nrefs=0,width=100": "inter_recon_chroma_refs: nrefs 0 out of [1,8]",
        "fenc=NULL,nrefs=0": "inter_recon_chroma_refs: NULL operand",
        "tables,fenc=NULL": "inter_recon_chroma_refs: " + _NO_TABLES,
        "width=100": "inter_recon_chroma_refs: width/height (luma) must be multiples of 64",
        "height=-64": "inter_recon_chroma_refs: width/height (luma) must be multiples of 64",
        "depth=9": "inter_recon_chroma_refs: depth 9",
        "level=-1": "inter_recon_chroma_refs: level -1 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "level=3": "inter_recon_chroma_refs: level 3 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "qp=-1": "inter_recon_chroma_refs: qp -1 out of range",
        "depth=10,qp=64": "inter_recon_chroma_refs: qp 64 out of range",
    },
    "x265hip_inter_recon_chroma_pair_refs": {
        "cb:tables": "inter_recon_chroma_refs: " + _NO_TABLES,
        "cb:fenc=NULL": "inter_recon_chroma_refs: NULL operand",
        "cb:ref_idx=NULL": "inter_recon_chroma_refs: NULL operand",
        "cb:nrefs=9": "inter_recon_chroma_refs: nrefs 9 out of [1,8]",
        "cb:plane3=NULL": "inter_recon_chroma_refs: NULL plane of reference 3",
        "cb:nrefs=0,width=100": "inter_recon_chroma_refs: nrefs 0 out of [1,8]",
        "cb:fenc=NULL,nrefs=0": "inter_recon_chroma_refs: NULL operand",
        "cb:tables,fenc=NULL": "inter_recon_chroma_refs: " + _NO_TABLES,
        "cb:width=100": "inter_recon_chroma_refs: width/height (luma) must be multiples of 64",
        "cb:height=-64": "inter_recon_chroma_refs: width/height (luma) must be multiples of 64",
        "cb:depth=9": "inter_recon_chroma_refs: depth 9",
        "cb:level=-1": "inter_recon_chroma_refs: level -1 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "cb:level=3": "inter_recon_chroma_refs: level 3 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "cb:qp=-1": "inter_recon_chroma_refs: qp -1 out of range",
        "cb:depth=10,qp=64": "inter_recon_chroma_refs: qp 64 out of range",
        "cr:tables": "inter_recon_chroma_refs: " + _NO_TABLES,
        "cr:fenc=NULL": "inter_recon_chroma_refs: NULL operand",
        "cr:ref_idx=NULL": "inter_recon_chroma_refs: NULL operand",
        "cr:nrefs=9": "inter_recon_chroma_refs: nrefs 9 out of [1,8]",
        "cr:plane3=NULL": "inter_recon_chroma_refs: NULL plane of reference 3",
        "cr:nrefs=0,width=100": "inter_recon_chroma_refs: nrefs 0 out of [1,8]",
        "cr:fenc=NULL,nrefs=0": "inter_recon_chroma_refs: NULL operand",
        "cr:tables,fenc=NULL": "inter_recon_chroma_refs: " + _NO_TABLES,
        "cr:width=100": "inter_recon_chroma_refs: width/height (luma) must be multiples of 64",
        "cr:height=-64": "inter_recon_chroma_refs: width/height (luma) must be multiples of 64",
        "cr:depth=9": "inter_recon_chroma_refs: depth 9",
        "cr:level=-1": "inter_recon_chroma_refs: level -1 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "cr:level=3": "inter_recon_chroma_refs: level 3 (0..2 = 8x8, 16x16, 32x32 luma blocks)",
        "cr:qp=-1": "inter_recon_chroma_refs: qp -1 out of range",
        "cr:depth=10,qp=64": "inter_recon_chroma_refs: qp 64 out of range",
        "cb:NULL record": "inter_recon_chroma_refs: NULL operand",
        "cr:NULL record": "inter_recon_chroma_refs: NULL operand",
        "both:NULL record": "inter_recon_chroma_refs: NULL operand",
        "cr:level=1": "inter_recon_chroma_refs: " + _DIFFER + "nrefs",
        "cr:width=64": "inter_recon_chroma_refs: " + _DIFFER + "nrefs",
        "cr:height=128": "inter_recon_chroma_refs: " + _DIFFER + "nrefs",
        "cr:depth=10": "inter_recon_chroma_refs: " + _DIFFER + "nrefs",
        "cr:nrefs=3": "inter_recon_chroma_refs: " + _DIFFER + "nrefs",
    },
    "x265hip_tu_launch_grid": {
        "-1,16,8,0,1,100": "tu_launch_grid: entry -1",
        "5,16,8,0,1,100": "tu_launch_grid: entry 5",
        "7,16,8,0,1,100": "tu_launch_grid: entry 7",
        "10,16,8,0,1,100": "tu_launch_grid: entry 10",
        "0,4,8,0,1,100": "tu_launch_grid: transform size 4 for entry 0",
        "0,64,8,0,1,100": "tu_launch_grid: transform size 64 for entry 0",
        "1,4,8,0,1,100": "tu_launch_grid: transform size 4 for entry 1",
        "2,32,8,0,1,100": "tu_launch_grid: transform size 32 for entry 2",
        "3,32,8,0,1,100": "tu_launch_grid: transform size 32 for entry 3",
        "4,2,8,0,1,100": "tu_launch_grid: transform size 2 for entry 4",
        "8,4,8,0,1,100": "tu_launch_grid: transform size 4 for entry 8",
        "9,32,8,0,1,100": "tu_launch_grid: transform size 32 for entry 9",
        "0,16,9,0,1,100": "tu_launch_grid: depth 9",
        "0,16,16,0,1,100": "tu_launch_grid: depth 16",
        "8,16,8,1,1,100": "tu_launch_grid: entry 8 takes no tables",
        "9,16,8,1,2,100": "tu_launch_grid: entry 9 takes no tables",
        "0,16,8,0,2,100": "tu_launch_grid: 2 planes for entry 0",
        "1,16,8,0,2,100": "tu_launch_grid: 2 planes for entry 1",
        "3,16,8,0,2,100": "tu_launch_grid: 2 planes for entry 3",
        "4,16,8,0,2,100": "tu_launch_grid: 2 planes for entry 4",
        "8,16,8,0,2,100": "tu_launch_grid: 2 planes for entry 8",
        "2,16,8,0,3,100": "tu_launch_grid: 3 planes for entry 2",
        "9,16,8,0,0,100": "tu_launch_grid: 0 planes for entry 9",
        "0,16,8,0,1,0": "tu_launch_grid: nblocks 0",
        "2,16,8,1,2,-5": "tu_launch_grid: nblocks -5",
    },
}
# the chroma flavour of the bi-predictive stage goes through the same launcher and names itself like the luma one
EXPECT["x265hip_inter_recon_chroma_bi"] = EXPECT["x265hip_inter_recon_bi"]
