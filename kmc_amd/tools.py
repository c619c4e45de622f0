"""python -m kmc_amd.tools simple <db1> [-ci<v> -cx<v>] <db2> [-ci<v> -cx<v>] <operation> <out> [-ci<v> -cx<v> -cs<v> -oc<mode>] [<operation> <out> ...]

`kmc_tools simple` on the device: the argument order and the defaults are the reference's (kmc_tools/parameters_parser.cpp), the databases written are
byte for byte those kmc_tools writes. One kmc_hip_db_set_op_device call per output; an input as `kmc` wrote it (KMC2) is ordered on the device first."""
from __future__ import annotations

import sys

import numpy as np

from . import capi, dbio


class UsageError(SystemExit):
    def __init__(self, msg):
        super().__init__("kmc_amd.tools: " + msg)


def _num(arg: str, name: str) -> int:
    try:
        return int(arg[len(name):])
    except ValueError:
        raise UsageError(f"bad value in {arg}")


def parse_simple(argv):
    """-> ([(path, ci, cx)] x 2, [dict(op, path, ci, cx, cs, oc)]); 0 = not given"""
    pos = 0
    inputs = []
    for _ in range(2):
        if pos >= len(argv) or argv[pos].startswith("-"):
            raise UsageError("simple needs two input databases")
        path, ci, cx = argv[pos], 0, 0
        pos += 1
        while pos < len(argv) and argv[pos].startswith("-"):
            if argv[pos].startswith("-ci"):
                ci = _num(argv[pos], "-ci")
            elif argv[pos].startswith("-cx"):
                cx = _num(argv[pos], "-cx")
            else:
                raise UsageError(f"unknown input option {argv[pos]}")
            pos += 1
        inputs.append((path, ci, cx))
    outputs = []
    while pos < len(argv):
        op = argv[pos]
        if op not in capi.DB_OPS:
            raise UsageError(f"unknown operation {op} (one of {', '.join(capi.DB_OPS)})")
        if pos + 1 >= len(argv):
            raise UsageError(f"{op} needs an output database")
        o = dict(op=op, path=argv[pos + 1], ci=0, cx=0, cs=0, oc=None)
        pos += 2
        while pos < len(argv) and argv[pos].startswith("-"):
            a = argv[pos]
            if a.startswith("-ci"):
                o["ci"] = _num(a, "-ci")
            elif a.startswith("-cx"):
                o["cx"] = _num(a, "-cx")
            elif a.startswith("-cs"):
                o["cs"] = _num(a, "-cs")
            elif a.startswith("-oc"):
                if a[3:] not in capi.DB_COUNTER_OPS:
                    raise UsageError(f"unknown counter mode {a} (-ocmin, -ocmax, -ocsum, -ocdiff, -ocleft, -ocright)")
                o["oc"] = a[3:]
            elif a.startswith("-o"):
                if a[2:] != "kmc":
                    raise UsageError(f"{a}: KFF output is not written, only KMC databases")
            else:
                raise UsageError(f"unknown output option {a}")
            pos += 1
        outputs.append(o)
    if not outputs:
        raise UsageError("simple needs at least one <operation> <out>")
    return inputs, outputs


DEFAULT_COUNTER_OP = {"intersect": "min", "union": "sum"}  # config.h:96-110; every other operation: diff


class _DeviceDb:
    """an input's KMC1 body in HBM"""

    def __init__(self, ctx, db: dbio.Database):
        self.ctx, self.db = ctx, db
        self.allocs = []
        if db.kmc2:
            self._order(db)
        else:
            self.p, self.n = db.lut_prefix_len, db.total_kmers
            self.d_recs, self.d_lut = self._up(db.recs), self._up(db.lut)

    def _up(self, a: np.ndarray) -> int:
        d = self.ctx.malloc(a.nbytes + 256)
        self.allocs.append(d)
        if a.nbytes:
            self.ctx.h2d(d, np.ascontiguousarray(a))
        return d

    def _order(self, db):
        ctx = self.ctx
        p_in = capi.make_params(db.kmer_len, both_strands=int(db.both_strands), cutoff_min=max(db.min_count, 1), cutoff_max=db.max_count,
                                counter_max=(1 << (8 * db.counter_size)) - 1, lut_prefix_len=db.lut_prefix_len)
        assert ctx.out_rec_bytes(p_in) == db.rec_bytes
        descs = (capi.BinDesc * max(len(db.bins), 1))()
        for i, (recs, lut) in enumerate(db.bins):
            d_small = self._up(np.array([0, 0, 0, 0, recs.size, 0, 0, 0], dtype=np.uint64))
            descs[i] = capi.BinDesc(0, 0, 0, 0, 0, self._up(recs), recs.size, d_small + 32, self._up(lut), d_small)
        self.p = dbio.best_lut_prefix_len(db.kmer_len, db.total_kmers)
        rb = (db.kmer_len - self.p) // 4 + db.counter_size
        self.d_recs, self.d_lut = ctx.malloc(db.total_kmers * rb + 256), ctx.malloc(8 << (2 * self.p))
        self.allocs += [self.d_recs, self.d_lut]
        descs_n = (capi.BinDesc * len(db.bins))(*descs[: len(db.bins)])
        self.n = ctx.order_database_device(p_in, descs_n, self.p, self.d_recs, db.total_kmers * rb, self.d_lut)

    def view(self, ci: int, cx: int) -> capi.DbView:
        return capi.DbView(self.d_recs, self.n, self.d_lut, self.p, self.db.counter_size, ci, cx)

    def free(self):
        for d in self.allocs:
            self.ctx.free(d)
        self.allocs = []


def simple(argv, ctx=None) -> list:
    """Runs the command line; returns per output the dict of tallies of kmc_hip_db_set_op_device."""
    inputs, outputs = parse_simple(argv)
    dbs = []
    for path, _, _ in inputs:
        try:
            dbs.append(dbio.read_database(path))
        except dbio.DbFormatError as e:
            raise UsageError(str(e))
    if dbs[0].kmer_len != dbs[1].kmer_len:
        raise UsageError(f"the inputs have different k-mer lengths ({dbs[0].kmer_len} and {dbs[1].kmer_len})")
    for (path, _, _), db in zip(inputs, dbs):
        if db.counter_size == 0:
            raise UsageError(f"{path}: counter size 0 (a k-mer set without counters) is not supported, as in kmc_tools")
    k = dbs[0].kmer_len
    # parameters_parser.cpp:842-866
    eff = [(ci or db.min_count, cx or db.max_count) for (_, ci, cx), db in zip(inputs, dbs)]
    def_ci, def_cx = min(e[0] for e in eff), max(e[1] for e in eff)
    def_cs = (1 << (8 * max(db.counter_size for db in dbs))) - 1
    p_out = max(dbio.best_lut_prefix_len(k, db.total_kmers) for db in dbs)  # kmc1_db_writer.h:425-456
    canonical = all(db.both_strands for db in dbs)
    own = ctx is None
    if own:
        ctx = capi.Context((0,))
    dev = []
    results = []
    try:
        dev = [_DeviceDb(ctx, db) for db in dbs]
        views = [d.view(*e) for d, e in zip(dev, eff)]
        n_a, n_b = dev[0].n, dev[1].n
        for o in outputs:
            ci, cx, cs = o["ci"] or def_ci, o["cx"] or def_cx, o["cs"] or def_cs
            cs_bytes = min(dbio.byte_log(cs), dbio.byte_log(cx))  # kmc1_db_writer.h:154
            oc = o["oc"] or DEFAULT_COUNTER_OP.get(o["op"], "diff")
            op = capi.DbOp(capi.DB_OPS[o["op"]], capi.DB_COUNTER_OPS[oc], ci, cs, cx, p_out)
            rb = (k - p_out) // 4 + cs_bytes
            bound = {"union": n_a + n_b, "intersect": min(n_a, n_b), "kmers_subtract": n_a, "counters_subtract": n_a}.get(o["op"], n_b)
            d_out, d_lut = ctx.malloc(bound * rb + 256), ctx.malloc(8 << (2 * p_out))
            try:
                n, st = ctx.db_set_op_device(k, views[0], views[1], op, d_out, bound * rb, d_lut)
                recs, lut = np.zeros(n * rb, dtype=np.uint8), np.zeros(1 << (2 * p_out), dtype=np.uint64)
                if n:
                    ctx.d2h(recs, d_out)
                ctx.d2h(lut, d_lut)
            finally:
                ctx.free(d_out)
                ctx.free(d_lut)
            dbio.write_kmc1(o["path"], k, cs_bytes, p_out, ci, cx, canonical, lut, recs, mode=dbs[0].mode)
            results.append(st)
    finally:
        for d in dev:
            d.free()
        if own:
            ctx.close()
    return results


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] != "simple":
        raise UsageError("usage: python -m kmc_amd.tools simple <db1> [-ci -cx] <db2> [-ci -cx] <operation> <out> [-ci -cx -cs -oc<mode>] ...")
    for (o, st) in zip(parse_simple(argv[1:])[1], simple(argv[1:])):
        print(f"{o['op']} -> {o['path']}: " + ", ".join(f"{a} {b}" for a, b in st.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
