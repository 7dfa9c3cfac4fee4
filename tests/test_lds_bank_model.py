"""tools/lds_bank_model.py: the LDS bank model behind the layout of the 2-D set kernels ("LDS layout of the 2-D
set kernels").  No GPU.

The machine rules are tried on cases small enough to check by hand; then, at P = 31 and P = 21 in two dimensions, the model
must show what the layout was built for: the old partner fetch (ds_read2_b64 of 8 bytes at a 16-byte stride) a 2-way conflict,
the new one (ds_read_b128, 256-byte aligned per-set stride, row slots without a row reading the copy at their own position)
free of conflicts in every round and both row slots, from every wavefront of the workgroup; struct size a multiple of 256 B;
the workgroup within half a CU's LDS.

Row reads: the lanes that read a row of the packed triangle are free of conflicts (16 consecutive triangular numbers are 16
different residues mod 16, and the sets' triangles are 16 doubles apart mod 32).  The one lane per set whose row slot holds the
data row, and at P = 21 the lanes whose slots read zeros, read from the data-row staging area, which lies where the struct has
room and not at the bank position of row P: the model counts 92 conflict cycles per wave-task for them at P = 31 and 61 at
P = 21 (of 278 and 207 row-read cycles), before and after this layout.  The test pins both figures: the triangle rows at 0,
the staging-area lanes at what they cost, so that neither moves unnoticed.  The 2-D lean kernels read their rows one column
per ds_read_b64 since (156 cycles, 62 of them conflicts, at P = 31): pinned too.  The model's totals at P = 31 are what the
counters of the headline read per wave-task (profiles/lds_layout_pmc_summary.json)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lds_bank_model", os.path.join(ROOT, "tools", "lds_bank_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


def test_machine_rules_on_hand_checkable_cases():
    lanes = range(64)
    # 64 lanes x 8 B, consecutive: 2 groups of 32 lanes cover the 64 banks once each
    assert M.cost("ds_read_b64", [8 * l for l in lanes]) == (2, 0)
    # every lane the same address: broadcast
    assert M.cost("ds_read_b64", [1000 for _ in lanes]) == (2, 0)
    # 8 B at a 16-B stride: lanes l and l + 16 of a 32-lane group meet on a bank (64 banks = 256 B), 2-way
    assert M.cost("ds_read_b64", [16 * l for l in lanes]) == (4, 2)
    # ds_read2_b64 offset0:2k offset1:2k+1 at a 16-B stride: each access 4 x 16 lanes over 32 banks (128 B): lanes l and l + 8
    assert M.cost("ds_read2_b64", [(16 * l, 16 * l + 8) for l in lanes]) == (16, 8)
    # the same as two adjacent doubles at an 8-B lane stride (a row read): 16 lanes x 8 B = 128 B, no conflict
    assert M.cost("ds_read2_b64", [(8 * l, 8 * l + 8 * 64) for l in lanes]) == (8, 0)
    # ds_read_b128, consecutive 16-byte rows: a group's 16 lanes cover 256 B once whatever lanes they are
    assert M.cost("ds_read_b128", [16 * l for l in lanes]) == (4, 0)
    # ... but the group {0-3, 12-15, 20-27} mixes two 16-lane sets: set strides of 736 B (not a multiple of 256) make them overlap
    assert M.cost("ds_read_b128", [736 * (l // 16) + 16 * (l % 16) for l in lanes])[1] > 0
    assert M.cost("ds_read_b128", [768 * (l // 16) + 16 * (l % 16) for l in lanes]) == (4, 0)
    # lane 15 of a set 256 B behind its lane 0 (row 16 + s against row 0 + s): the same banks, 2-way in every group
    assert M.cost("ds_read_b128", [768 * (l // 16) + (16 * (l % 16) if l % 16 != 15 else 256) for l in lanes]) == (8, 4)
    # stores: 4 x 16 lanes over 32 banks; masked lanes take no part; array cycles below the 6 issue cycles cost nothing
    assert M.cost("ds_write_b64", [8 * l for l in lanes]) == (4, 0)
    assert M.cost("ds_write_b64", [16 * l if l < 16 else None for l in lanes]) == (5, 1)
    assert M.store_time("ds_write_b64", 5) == 6 and M.store_time("ds_write_b64", 8) == 8
    with pytest.raises(AssertionError):
        M.cost("ds_read_b128", [16 * l + 8 for l in lanes])


def test_geometry_and_layout_formulas():
    g = M.Geo(31)
    assert (g.RPL, g.LPS, g.SLOTS, g.SPW, g.ZROW) == (2, 16, 32, 4, True)
    old, new = M.Layout(31, 2, False), M.Layout(31, 2, True)
    assert (old.TRI, old.COLS, old.XYROWS, old.XYLEN, old.size, old.workgroup) == (496, 34, 46, 92, 20184, 80736)
    assert (new.XYROWS, new.XYLEN, new.xy_off, new.col_off, new.size) == (47, 96, 15872, 18944, 20480)
    new21 = M.Layout(21, 2, True)
    assert (new21.XYROWS, new21.XYLEN) == (32 + 10, 96)        # copies up to row SLOTS - 1 + P/2
    for d in (1, 3):                                           # one and three dimensions: the same layout either way
        a, b = M.Layout(31, d, False), M.Layout(31, d, True)
        assert (a.size, a.xy_off, a.col_off, a.XYLEN) == (b.size, b.xy_off, b.col_off, b.XYLEN)
    assert M.Layout(31, 1, False).workgroup == 74848


@pytest.mark.parametrize("P", [31, 21])
def test_old_fetch_is_two_way_new_fetch_is_conflict_free(P):
    old, new = M.Layout(P, 2, False), M.Layout(P, 2, True)
    for wave in range(4):                                      # the four wavefronts sit at four offsets of the workgroup's LDS
        for s in range(1, P // 2 + 1):
            # first row slot, every lane owns a row: 2 accesses x 4 groups x 2-way
            assert M.cost("ds_read2_b64", M.fetch_addrs(old, 0, s, wave)) == (16, 8), (wave, s)
            assert M.cost("ds_read2_b64", M.fetch_addrs(old, 1, s, wave))[1] >= 8, (wave, s)
            for q in range(2):
                addrs = M.fetch_addrs(new, q, s, wave)
                assert all(a % 16 == 0 for a in addrs)
                assert M.cost("ds_read_b128", addrs) == (4, 0), (wave, q, s)
    _, parts_old = M.task_model(P, False)
    _, parts_new = M.task_model(P, True)
    H = P // 2
    assert parts_old["partner fetches"]["instructions"] == parts_new["partner fetches"]["instructions"] == 2 * H
    assert parts_new["partner fetches"] == dict(instructions=2 * H, cycles=8 * H, conflict=0, time=8 * H)
    assert parts_old["partner fetches"]["conflict"] >= 16 * H
    # every fetched row lies inside the set's coordinates, and a copy is what it copies: row r + s <= SLOTS - 1 + P/2
    assert new.XYROWS * 16 <= new.XYLEN * 8 and new.XYROWS == new.G.SLOTS + H


@pytest.mark.parametrize("P", [31, 21])
def test_row_reads(P):
    for wide in (False, True):
        L = M.Layout(P, 2, wide)
        tri_conf = stag_conf = 0
        for q in range(2):
            tri_lane = [on and i + q * 16 < P for _, _, i, on, _ in M._lanes(L)]
            for name, addrs in M.row_read_instrs(L, q, "read2_b64"):
                tri_conf += M.cost(name, [a if t else None for a, t in zip(addrs, tri_lane)])[1]
                stag_conf += M.cost(name, addrs)[1]
        assert tri_conf == 0                                   # the rows of the triangle: conflict-free
        assert stag_conf == {31: 92, 21: 62 if not wide else 61}[P]   # with the lanes that read the data row / zeros
    # one column per instruction: the 64-bank ds_read_b64 serves two sets per group, their triangles 16 doubles apart mod 32
    # (P = 31: TRI = 496 = 16 mod 32; at P = 21, TRI = 232 = 8 mod 32, the two sets of a group overlap and this form conflicts)
    L = M.Layout(P, 2, True)
    conf = 0
    for q in range(2):
        tri_lane = [on and i + q * 16 < P for _, _, i, on, _ in M._lanes(L)]
        for name, addrs in M.row_read_instrs(L, q, "read_b64"):
            conf += M.cost(name, [a if t else None for a, t in zip(addrs, tri_lane)])[1]
    assert (L.TRI % 32, conf == 0) == {31: (16, True), 21: (8, False)}[P]
    # what the 2-D lean kernels do since (GPV_OPT_ROWB64): all lanes, data-row and zero lanes included
    rows = M.task_model(P, True)[1]["row reads"]
    assert (rows["instructions"], rows["cycles"], rows["conflict"]) == {31: (47, 156, 62), 21: (37, 127, 53)}[P]


@pytest.mark.parametrize("P", [31, 26, 21])
def test_sizes(P):
    old, new = M.Layout(P, 2, False), M.Layout(P, 2, True)
    assert new.size % 256 == 0 and new.xy_off % 256 == 0 and (new.XYLEN * 8) % 256 == 0
    assert new.waves == 4 and new.workgroup <= 81920
    assert new.blocks_per_cu == old.blocks_per_cu == 2


def test_every_built_row_length_keeps_its_occupancy():
    for P in (4, 8, 11, 16, 21, 26, 31, 32, 41, 51, 61, 64):
        old, new = M.Layout(P, 2, False), M.Layout(P, 2, True)
        assert (new.waves, new.blocks_per_cu) == (old.waves, old.blocks_per_cu), P
        assert new.XEXT <= P                                   # every copied row is a row


def test_staging_stores_keep_their_conflicts():
    """the staging stores are left alone: the model's figure for them, on record (P = 31: the same before and after)"""
    _, old = M.task_model(31, False)
    _, new = M.task_model(31, True)
    assert old["staging stores"] == new["staging stores"]
    assert new["staging stores"]["instructions"] == 30 and new["staging stores"]["cycles"] == 260
