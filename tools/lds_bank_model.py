"""LDS bank model of one unpadded task of the lean 2-D set kernel, for the layout before and after the wide coordinate reads.

    python tools/lds_bank_model.py [P ...]               # default: 31 26 21 (two dimensions)

Pure Python, no GPU.  The machine model is the LDS table of the CDNA4 microarchitecture notes: a wave64 LDS instruction is
served in fixed lane groups, one LDS cycle per group when conflict-free; only lanes of one group conflict, lanes with the same
address share one access (broadcast), and every further distinct address on a busy bank adds a cycle to that group.

    instruction    lane groups                                   banks (4 B)   cycles, conflict-free
    ds_read_b64    {0-31} {32-63}                                64            2
    ds_read_b128   {0-3,12-15,20-27} {4-11,16-19,28-31} (+32)    64            4
    ds_read2_b64   two accesses, each 4 x 16 contiguous lanes    32            8
    ds_write_b64   4 x 16 contiguous lanes                       32            4 in the array; 6 to issue (address + data transfer)

A store's conflict costs time only once its array cycles exceed the 6 cycles its operands take to reach the LDS; the model
reports array cycles and max(6, array cycles) for stores.  Identical store addresses (the shadow lanes of the rounds write the
bits another lane writes, row slots without a cell write a dump cell) are counted as one access, like reads.

The layout formulas repeat SetsLdsDims / SetsLds and Geo of gpvecchia_amd/csrc/gpv_sets_kernel.hpp for the closed-form families
(keep them equal; tests/test_lds_wide_reads_build.py compares the workgroup sizes with the built kernels').
"""
import sys

NSUMS = 8
LDS_PER_CU = 163840
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS = B128_GROUPS + [[l + 32 for l in g] for g in B128_GROUPS]
HALVES = [list(range(0, 32)), list(range(32, 64))]
QUARTERS = [list(range(16 * g, 16 * g + 16)) for g in range(4)]
# name: (lane groups, accesses per instruction, bytes per access, banks, issue cycles of a store or None)
INSTR = {"ds_read_b64": (HALVES, 1, 8, 64, None), "ds_read_b128": (B128_GROUPS, 1, 16, 64, None),
         "ds_read2_b64": (QUARTERS, 2, 8, 32, None), "ds_write_b64": (QUARTERS, 1, 8, 32, 6)}


def cost(instr, addrs):
    """(cycles, conflict cycles) in the LDS array of one wave instruction.  addrs: 64 entries, one per lane: a byte address,
    a tuple of byte addresses (one per access: ds_read2_b64), or None for a lane that is masked off."""
    groups, nacc, width, banks, _ = INSTR[instr]
    cycles = conflict = 0
    for acc in range(nacc):
        for g in groups:
            on_bank = {}
            for lane in g:
                a = addrs[lane]
                if a is None:
                    continue
                a = a[acc] if isinstance(a, tuple) else a
                assert a % min(width, 16) == 0 or instr != "ds_read_b128", "ds_read_b128 needs 16-byte alignment"
                for w in range(a // 4, (a + width) // 4):
                    on_bank.setdefault(w % banks, set()).add(w)
            ways = max([len(v) for v in on_bank.values()] + [1])
            cycles += ways
            conflict += ways - 1
    return cycles, conflict


def store_time(instr, array_cycles):
    return max(INSTR[instr][4], array_cycles)


class Geo:
    """Geo<P> of the kernel (default settings)"""

    def __init__(self, P):
        self.P = P
        self.DPP2 = 48 < P <= 64 and P > 32
        self.DPP = 11 <= P <= 48 or self.DPP2
        self.RPL = 2 if self.DPP2 else ((P + 15) // 16 if self.DPP else (2 if 24 <= P <= 41 else 1))
        lps0 = (P + self.RPL - 1) // self.RPL
        self.LPS = 32 if self.DPP2 else (16 if self.DPP else
                                         (lps0 + 1 if lps0 * self.RPL == P and lps0 < 64 and 64 // (lps0 + 1) == 64 // lps0 else lps0))
        self.SLOTS = self.LPS * self.RPL
        self.ZROW = self.SLOTS > P
        self.SPW = 64 // self.LPS
        self.MINW = 2 if P <= 32 else (1 if self.RPL >= 2 else 2)


class Layout:
    """SetsLds<P, D, closed-form Matern>: byte offsets inside a wavefront's struct.  wide: the layout with 16-byte coordinate
    reads (two dimensions only), else the one before it."""

    def __init__(self, P, D, wide):
        assert D in (1, 2, 3)
        g = self.G = Geo(P)
        self.P, self.D = P, D
        self.WIDE = bool(wide) and D == 2
        self.TRI = (P * (P + 1) // 2 + 1) & ~1
        self.DS = 4 if D == 3 else D
        cols0 = (g.SLOTS + 2) & ~1
        self.COLS = cols0 + 2 if (cols0 * 8) % 256 == 0 else cols0
        self.NCOL = 1 if g.DPP else 2
        self.XEXT = P // 2 + (g.SLOTS - P if self.WIDE else 0)
        self.XYROWS = P + self.XEXT
        xylen0 = 3 * self.XYROWS if D == 3 else self.XYROWS * self.DS
        self.XYLEN = (xylen0 + 31) & ~31 if self.WIDE else xylen0
        self.NEEDZERO = g.SLOTS > P + (1 if g.ZROW else 0)
        tri = g.SPW * self.TRI * 8
        col = self.NCOL * g.SPW * self.COLS * 8
        xy = g.SPW * self.XYLEN * 8
        tail = (self.COLS if self.NEEDZERO else 2) * 8 + g.SPW * NSUMS * 8 + 8          # zero, acc, ix
        self.tri_off = 0
        if self.WIDE:                                        # tri, xy (256-B aligned), col, zero, acc, ix; 256-B aligned struct
            self.xy_off = (tri + 255) & ~255
            self.col_off = self.xy_off + xy
            self.zero_off = self.col_off + col
            self.size = (self.zero_off + tail + 255) & ~255
        else:                                                # tri, col, xy, zero, acc, ix; 8-B aligned
            self.col_off = tri
            self.xy_off = tri + col
            self.zero_off = self.xy_off + xy
            self.size = self.zero_off + tail
        self.waves = 1 if self.size * 8 > LDS_PER_CU else 4
        self.workgroup = self.size * self.waves
        self.blocks_per_cu = max(1, min(LDS_PER_CU // self.workgroup, (4 * g.MINW) // self.waves))

    def set_stride_xy(self):
        return self.XYLEN * 8


def _lanes(L, wave=0):
    g = L.G
    base = wave * L.size
    for lane in range(64):
        sub = lane // g.LPS
        on = sub < g.SPW
        yield lane, (sub if on else g.SPW - 1), (lane - sub * g.LPS if on else 0), on, base


def fetch_addrs(L, q, s, wave=0):
    """partner coordinates of round s, row slot q: lane of row r reads row r + s (rows >= P: the copies); a slot without a row
    reads the partners of row 0 (wide layout: it shadows row r - P and reads the partners of its copy, row r)"""
    out = []
    for lane, sub, i, on, base in _lanes(L, wave):
        r = i + q * L.G.LPS
        row = r if (on and (r < L.P or L.WIDE)) else 0
        a = base + L.xy_off + sub * L.XYLEN * 8 + (row + s) * 16
        out.append(a if L.WIDE else (a, a + 8))
    return out


def stage_addrs(L, q, s, wave=0):
    """where the pair (r, r + s mod P) is staged in the packed triangle (slots without a row: the pair of the row they shadow)"""
    P, out = L.P, []
    for lane, sub, i, on, base in _lanes(L, wave):
        r = i + q * L.G.LPS
        r = r if (on and r < P) else (r - P if (on and L.WIDE) else 0)
        rt = r * (r + 1) // 2
        idx = rt + r * (s + 1) + s * (s + 1) // 2 if r < P - s else rt + (r + s - P)
        out.append(base + L.tri_off + (sub * L.TRI + idx) * 8)
    return out


def row_base(L, q, lane_info, padded_rows=False):
    lane, sub, i, on, base = lane_info
    P, g = L.P, L.G
    r = i + q * g.LPS
    if on and r < P:
        rt = sum((k + 2) & ~1 for k in range(r)) if padded_rows else r * (r + 1) // 2
        return base + L.tri_off + (sub * L.TRI + rt) * 8
    if on and r == P:
        return base + L.col_off + ((L.NCOL - 1) * g.SPW + sub) * L.COLS * 8      # the data row
    return base + L.zero_off


def lik_maxcol(L, q):
    return min((q + 1) * L.G.LPS - 1, L.P - 1)


def row_read_instrs(L, q, how, wave=0):
    """[(instruction, addrs)] that load columns 0 .. lik_maxcol(q) of the lane's row.  how: 'read2_b64' (what hipcc makes of
    the source: pairs of adjacent columns), 'read_b64' (one column per instruction), 'read_b128' (pairs of columns from rows
    padded to an even length, 16-byte aligned: a layout that is not built)"""
    ncol = lik_maxcol(L, q) + 1
    info = list(_lanes(L, wave))
    bases = [row_base(L, q, li, padded_rows=(how == "read_b128")) for li in info]
    out = []
    if how == "read_b64":
        return [("ds_read_b64", [b + 8 * c for b in bases]) for c in range(ncol)]
    for c in range(0, ncol - 1, 2):
        if how == "read2_b64":
            out.append(("ds_read2_b64", [(b + 8 * c, b + 8 * c + 8) for b in bases]))
        else:
            out.append(("ds_read_b128", [b + 8 * c for b in bases]))
    if ncol % 2:
        out.append(("ds_read_b64", [b + 8 * (ncol - 1) for b in bases]))
    return out


def staging_instrs(L, wave=0):
    """the straight path's other LDS traffic: coordinates of the own row and its copy (two 8-byte stores each), diagonal cell,
    data-row cell, and the last slot's read-back of its coordinates.  Slots without a cell store to the set's dump cell where
    a set has at most two of them (P = 31), else they are masked off."""
    P, g = L.P, L.G
    dumpable = g.SLOTS - P <= 2
    out = []
    for q in range(g.RPL):
        xy, xyx, dg, zz, back = [], [], [], [], []
        for lane, sub, i, on, base in _lanes(L, wave):
            r = i + q * g.LPS
            own = on and r < P
            zr0 = base + L.col_off + ((L.NCOL - 1) * g.SPW + sub) * L.COLS * 8
            dump = zr0 + 8 * g.SLOTS if dumpable else None
            xo = base + L.xy_off + sub * L.XYLEN * 8 + (r if (own or (on and L.WIDE)) else 0) * 16
            xy.append(xo if own else dump)
            xyx.append(xo + P * 16 if (own and r < L.XEXT) else dump)
            dg.append(base + (sub * L.TRI + r * (r + 1) // 2 + r) * 8 if own else dump)
            zz.append(zr0 + r * 8 if (own and r != P - 1) else dump)
            back.append((xo, xo + 8))
        for t in range(2):
            out.append(("ds_write_b64", [None if a is None else a + 8 * t for a in xy]))
        if q * g.LPS < L.XEXT:
            for t in range(2):
                out.append(("ds_write_b64", [None if a is None else a + 8 * t for a in xyx]))
        out.append(("ds_write_b64", dg))
        out.append(("ds_write_b64", zz))
        if (q + 1) * g.LPS > P:
            out.append(("ds_read2_b64", back))
    return out


def _sum(instrs):
    cyc = conf = time = 0
    for name, addrs in instrs:
        c, k = cost(name, addrs)
        cyc += c
        conf += k
        time += store_time(name, c) if INSTR[name][4] else c
    return dict(instructions=len(instrs), cycles=cyc, conflict=conf, time=time)


def task_model(P, wide, rows=None, wave=0):
    """LDS cycles of one unpadded wave-task (two dimensions), by part.  rows: how the matrix rows are read (row_read_instrs);
    default: what the kernel of that layout does (before: pairs of columns, after: one column per instruction)"""
    L = Layout(P, 2, wide)
    rows = rows or ("read_b64" if L.WIDE else "read2_b64")
    g, H = L.G, P // 2
    fetch = "ds_read_b128" if L.WIDE else "ds_read2_b64"
    parts = {
        "partner fetches": _sum([(fetch, fetch_addrs(L, q, s, wave)) for q in range(g.RPL) for s in range(1, H + 1)]),
        "staging stores": _sum([("ds_write_b64", stage_addrs(L, q, s, wave)) for q in range(g.RPL) for s in range(1, H + 1)]),
        "row reads": _sum([i for q in range(g.RPL) for i in row_read_instrs(L, q, rows, wave)]),
        "coordinate, diagonal and data-row staging": _sum(staging_instrs(L, wave)),
    }
    parts["total"] = {k: sum(p[k] for p in parts.values()) for k in ("instructions", "cycles", "conflict", "time")}
    return L, parts


def main(argv):
    for P in [int(a) for a in argv[1:]] or [31, 26, 21]:
        for wide in (False, True):
            L, parts = task_model(P, wide)
            print(f"P = {P}, D = 2, {'wide (16-byte) coordinate reads, rows by single columns' if wide else 'layout before the wide reads'}: "
                  f"struct {L.size} B, per-set xy stride {L.set_stride_xy()} B, workgroup {L.workgroup} B ({L.waves} waves), "
                  f"{L.blocks_per_cu} workgroups per CU")
            print(f"  {'part':44s} {'instr':>6s} {'array cycles':>13s} {'conflict':>9s} {'cycles with store issue':>24s}")
            for name, p in parts.items():
                print(f"  {name:44s} {p['instructions']:6d} {p['cycles']:13d} {p['conflict']:9d} {p['time']:24d}")
        for how in ("read2_b64", "read_b64", "read_b128"):
            L, parts = task_model(P, True, rows=how)
            p = parts["row reads"]
            note = ""
            if how == "read_b128":
                grow = sum((k + 2) & ~1 for k in range(P)) - L.TRI
                fits = (L.size + L.G.SPW * grow * 8) * L.waves * 2 <= LDS_PER_CU
                note = f"   (rows padded to even length: +{L.G.SPW * grow * 8} B per wave, two workgroups per CU {'fit' if fits else 'DO NOT FIT'})"
            print(f"  row reads as {how:10s}: {p['instructions']:3d} instructions, {p['cycles']:4d} cycles, {p['conflict']:3d} conflict{note}")


if __name__ == "__main__":
    main(sys.argv)
