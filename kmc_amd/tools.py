"""python -m kmc_amd.tools simple <db1> [-ci<v> -cx<v>] <db2> [-ci<v> -cx<v>] <operation> <out> [-ci<v> -cx<v> -cs<v> -oc<mode>] [<operation> <out> ...]
python -m kmc_amd.tools filter [-t | -hm] <db> [-ci<v> -cx<v>] <reads> [-ci<v> -cx<v> -fa|-fq] <out> [-fa|-fq]
python -m kmc_amd.tools transform <db> [-ci<v> -cx<v>] <oper> [-s] <out> [-ci<v> -cx<v> -cs<v> -okmc] [<oper> ...]
python -m kmc_amd.tools complex <operations_definition_file>
python -m kmc_amd.tools compare <db1> [-ci<v> -cx<v>] <db2> [-ci<v> -cx<v>]
python -m kmc_amd.tools check <db> [-ci<v> -cx<v>] <kmer>
python -m kmc_amd.tools info <db>
python -m kmc_amd.tools export <db> [-ci<v> -cx<v>] <out> [-ci<v> -cx<v> -cs<v>] [--sections]

`kmc_tools simple`, `kmc_tools filter`, `kmc_tools transform` and `kmc_tools complex` on the device: the argument order and the defaults are the reference's (kmc_tools/parameters_parser.cpp),
the databases, the reads and the text written are byte for byte those kmc_tools writes. simple: one kmc_hip_db_set_op_device call per output. filter: one
kmc_hip_db_query_reads_device call per part of the reads file. transform: the input uploaded once, then per output kmc_hip_db_reduce_device (reduce, compact, set_counts,
sort), kmc_hip_db_histogram_device, or kmc_hip_db_dump_device per part of the text. A database as `kmc` wrote it (KMC2) is ordered on the device first — by transform
only when an output needs the order. complex: every input the expression names uploaded once, then ONE kmc_hip_db_expr_device call for the whole expression.
Every <db> may be a KFF file (the name, or the name + '.kff', as kmc_tools takes it): its sections go up in one piece and kmc_hip_kff_import_device makes the body — one
ascending body where the mode needs the order, the file's own order under a segmented LUT otherwise. The outputs remain KMC databases and text.
compare: ONE kmc_hip_db_compare_device call on the two ordered bodies; it prints what kmc_tools prints and exits with its status. check: the k-mer as a line of a reads
buffer through kmc_hip_db_query_reads_device (check_kmers: a batch of them), kmc_tools' presence rule of this mode applied on the host. info: the headers as kmc_tools
prints them; no device is opened. With these the front end has every mode of the kmc_tools command line."""
from __future__ import annotations

import os
import re
import sys

import numpy as np

from . import capi, dbio, readsio


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


def _read_input(path: str):
    """a database, or a KFF file by kmc_tools' path rule (kmer_file_header.cpp:104-126) -> dbio.Database | dbio.KffFile"""
    if dbio.is_kff(path) and not os.path.exists(path + ".kmc_pre"):
        return dbio.read_kff(path)
    return dbio.read_database(path)


class _DeviceDb:
    """an input's KMC1 body in HBM"""

    def __init__(self, ctx, db, order: bool = True):
        """order False: a KMC2 body, or the sections of a KFF file, stay as they lie in the file, under a LUT of n_seg x 4^p global offsets and the closing entry (what
        transform's histogram and unordered dump read)"""
        self.ctx, self.db = ctx, db
        self.allocs = []
        self.n_seg = 1
        if isinstance(db, dbio.KffFile):
            self._import_kff(db, order)
        elif db.kmc2 and order:
            self._order(db)
        elif db.kmc2:
            self.p, self.n, self.n_seg = db.lut_prefix_len, db.total_kmers, (db.raw_lut.size - 1) >> (2 * db.lut_prefix_len)
            self.d_recs, self.d_lut = self._up(db.raw_recs), self._up(db.raw_lut)
        else:
            self.p, self.n = db.lut_prefix_len, db.total_kmers
            self.d_recs, self.d_lut = self._up(db.recs), self._up(db.lut)

    def _up(self, a: np.ndarray) -> int:
        d = self.ctx.malloc(a.nbytes + 256)
        self.allocs.append(d)
        if a.nbytes:
            self.ctx.h2d(d, np.ascontiguousarray(a))
        return d

    def _import_kff(self, db, order):
        """the sections' records up back to back in one piece; ordered: one ascending body for the prefix length of its size; otherwise the file's order, the smallest
        valid prefix length and one LUT segment per section"""
        ctx, k = self.ctx, db.kmer_len
        sec_n = [n for _, n in db.sections] or [0]
        n = sum(sec_n)
        self.p = dbio.best_lut_prefix_len(k, n if order else 0)
        self.n_seg = 1 if order else len(sec_n)
        rb = (k - self.p) // 4 + db.counter_size
        d_kff = ctx.malloc(n * db.rec_bytes + 256)
        try:
            if n:
                ctx.h2d(d_kff, db.records())
            self.d_recs, self.d_lut = ctx.malloc(n * rb + 256), ctx.malloc(8 * ((self.n_seg << (2 * self.p)) + 1))
            self.allocs += [self.d_recs, self.d_lut]
            self.n = ctx.kff_import_device(k, db.counter_size, d_kff, sec_n, order, self.p, self.d_recs, n * rb, self.d_lut)
        finally:
            ctx.free(d_kff)

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


OUTPUT_FORMATS = ("kmc1", "kff")


def _kff_parts(ctx, k, body: capi.DbView, n_seg, first, count, data_size):
    """records [first, first + count) of the body as KFF record bytes, part by part ($KMC_HIP_KFF_PART_MB of records a part, 64 by default): one
    kmc_hip_db_kff_export_device call and one copy to the host per part — what write_kff takes as one section"""
    rb = (k + 3) // 4 + data_size
    part_bytes = max(1, int(float(os.environ.get("KMC_HIP_KFF_PART_MB", "64")) * (1 << 20)))
    part = max(1, part_bytes // rb)
    if not count:
        return
    cap = min(part, count) * rb
    d_kff = ctx.malloc(cap + 256)
    try:
        for at in range(first, first + count, part):
            n_bytes = ctx.db_kff_export_device(k, body, n_seg, at, min(part, first + count - at), data_size, d_kff, cap)
            out = np.zeros(n_bytes, dtype=np.uint8)
            ctx.d2h(out, d_kff)
            yield out
    finally:
        ctx.free(d_kff)


def _write_body(ctx, fmt: str, path: str, k: int, body: capi.DbView, ci: int, cx: int, both_strands: bool, mode: int = 0, n_seg: int = 1, sections=None):
    """The one place an output body leaves the device. body: a view of the records an entry wrote (its cutoffs are not read). fmt "kmc1": records and LUT come down and
    `path`.kmc_pre / .kmc_suf are written (n_seg 1). fmt "kff": the records are framed on the device and only KFF bytes come down; `path`.kff is written, as the
    reference appends the extension (kff_db_writer.h:79), with one section — or, with `sections` = [(first record, records)], one per element."""
    if fmt not in OUTPUT_FORMATS:
        raise ValueError(f"an output body is written as one of {OUTPUT_FORMATS}, not {fmt!r}")
    n, p, cs = int(body.n_recs), int(body.lut_prefix_len), int(body.counter_size)
    if fmt == "kff":
        secs = [(0, n)] if sections is None else sections
        dbio.write_kff(path + ".kff", k, cs, both_strands, ci, cx, [_kff_parts(ctx, k, body, n_seg, first, count, cs) for first, count in secs])
        return
    assert n_seg == 1 and sections is None
    recs, lut = np.zeros(n * ((k - p) // 4 + cs), dtype=np.uint8), np.zeros(1 << (2 * p), dtype=np.uint64)
    if n:
        ctx.d2h(recs, body.d_recs)
    ctx.d2h(lut, body.d_lut)
    dbio.write_kmc1(path, k, cs, p, ci, cx, both_strands, lut, recs, mode=mode)


def simple(argv, ctx=None) -> list:
    """Runs the command line; returns per output the dict of tallies of kmc_hip_db_set_op_device."""
    inputs, outputs = parse_simple(argv)
    dbs = []
    for path, _, _ in inputs:
        try:
            dbs.append(_read_input(path))
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
    p_out = max(dbio.best_lut_prefix_len(k, db.total_kmers) for db in dbs)  # kmc1_db_writer.h:425-456; a KFF input's total_kmers is 0
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
                _write_body(ctx, "kmc1", o["path"], k, capi.DbView(d_out, n, d_lut, p_out, cs_bytes, ci, cx), ci, cx, canonical, mode=dbs[0].mode)
            finally:
                ctx.free(d_out)
                ctx.free(d_lut)
            results.append(st)
    finally:
        for d in dev:
            d.free()
        if own:
            ctx.close()
    return results


FILTER_USAGE = """usage: python -m kmc_amd.tools filter [-t | -hm] <db> [-ci<v> -cx<v>] <reads> [-ci<v> -cx<v> -fa|-fq] <out> [-fa|-fq]
  <db>     a KMC database or a KFF file; -ci / -cx: k-mers with a counter outside [ci, cx] count as absent (default: the database's own cutoffs)
  <reads>  a FASTQ (default, -fq) or FASTA (-fa) file, '.gz' or not, or @file with one file name per line;
           -ci / -cx: keep a read with ci <= k-mers found <= cx (defaults 2 and 1e9); with a '.' in the value a fraction [0, 1] of the read's k-mers (both or neither)
  -t       trim a read behind its last k-mer in front of the first one found fewer than -ci times; -hm: replace every base of such a k-mer by N
  <out>    -fa writes FASTA from FASTQ
A read shorter than k has no k-mers: kept like any other read by integer bounds, passed through by -hm, and dropped by -t and by fraction bounds (kmc_tools reads an
empty vector, or casts a negative number to unsigned, there)."""


def _fastq_bound(arg, state):
    """parameters_parser.cpp:27-56: a value with a '.' is a fraction in [0, 1]; -ci and -cx must be of one kind"""
    v = arg[3:]
    if "." in v:
        try:
            f = float(v)
        except ValueError:
            raise UsageError(f"bad value in {arg}")
        if not 0.0 <= np.float32(f) <= 1.0:
            raise UsageError(f"wrong value for fastq input parameter: {arg[:3]}")
        if state.get("kind") == "int":
            raise UsageError("both -ci, -cx must be specified as real number [0;1] or as integer")
        state["kind"] = "float"
        return np.float32(f)
    if state.get("kind") == "float":
        raise UsageError("both -ci, -cx must be specified as real number [0;1] or as integer")
    state["kind"] = "int"
    return _num(arg, arg[:3])


def parse_filter(argv):
    """-> dict(mode 'normal' | 'trim' | 'mask', db, db_ci, db_cx (0: not given), inputs [paths], ci, cx, use_float, in_fastq, out, out_fastq)"""
    pos, mode = 0, "normal"
    while pos < len(argv) and argv[pos].startswith("-"):  # parameters_parser.cpp:208-226
        if argv[pos].startswith("-hm"):
            mode = "mask"
        elif argv[pos].startswith("-t"):
            mode = "trim"
        else:
            raise UsageError(f"unknown parameter for filter operation: {argv[pos]}")
        pos += 1
    if pos >= len(argv):
        raise UsageError("filter needs an input database\n" + FILTER_USAGE)
    o = dict(mode=mode, db=argv[pos], db_ci=0, db_cx=0, ci=2, cx=1000000000, f_ci=np.float32(0.0), f_cx=np.float32(1.0), use_float=False, in_fastq=True)
    pos += 1
    while pos < len(argv) and argv[pos].startswith("-"):
        if argv[pos].startswith("-ci"):
            o["db_ci"] = _num(argv[pos], "-ci")
        elif argv[pos].startswith("-cx"):
            o["db_cx"] = _num(argv[pos], "-cx")
        else:
            raise UsageError(f"unknown input option {argv[pos]}")
        pos += 1
    if pos >= len(argv):
        raise UsageError("Input fastq files(s) missed")
    name = argv[pos]
    pos += 1
    if name.startswith("@"):
        try:
            with open(name[1:]) as f:
                o["inputs"] = [ln.rstrip("\n") for ln in f if ln.rstrip("\n")]
        except OSError:
            raise UsageError(f"No {name[1:]} file")
    else:
        o["inputs"] = [name]
    state = {}
    while pos < len(argv) and argv[pos].startswith("-"):  # parameters_parser.cpp:129-158
        a = argv[pos]
        if a.startswith("-ci"):
            v = _fastq_bound(a, state)
            o["f_ci" if state["kind"] == "float" else "ci"] = v
        elif a.startswith("-cx"):
            v = _fastq_bound(a, state)
            o["f_cx" if state["kind"] == "float" else "cx"] = v
        elif a in ("-fa", "-fq"):
            o["in_fastq"] = a == "-fq"
        else:
            raise UsageError(f"unknown parameter {a}")
        pos += 1
    o["use_float"] = state.get("kind") == "float"
    o["out_fastq"] = o["in_fastq"]
    if pos >= len(argv):
        raise UsageError("Output fastq source missed")
    o["out"] = argv[pos]
    pos += 1
    while pos < len(argv):  # parameters_parser.cpp:176-205
        a = argv[pos]
        if a in ("-fa", "-fq"):
            o["out_fastq"] = a == "-fq"
            if not o["in_fastq"] and o["out_fastq"]:
                raise UsageError("cannot set -fq for output when -fa is set for input")
        elif a.startswith("-o"):
            raise UsageError(f"{a}: filter writes reads; neither a KMC database nor KFF is written")
        else:
            raise UsageError(f"Unknown parameter: {a}")
        pos += 1
    if o["use_float"] and mode != "normal":
        raise UsageError("trim (-t) and soft mask (-hm) are not compatibile with float values of cut off (-ci -cx)")
    return o


_LIT = np.frombuffer(b"\n+\n>", dtype=np.uint8)  # the bytes the helpers of fastq_filter.cpp:379-650 write themselves


def _filter_part(ctx, view, k, both, o, text) -> tuple:
    """one part of whole records -> (the bytes kmc_tools writes for it, reads in, reads out, the tallies)"""
    rec = readsio.parse(text, o["in_fastq"])
    n = len(rec)
    seq, off = readsio.sequence_buffer(rec)
    mode = o["mode"]
    allocs = []

    def dmalloc(nbytes):
        allocs.append(ctx.malloc(nbytes + 256))
        return allocs[-1]

    try:
        d_seq, d_off, d_cnt = dmalloc(seq.size), dmalloc(off.nbytes), dmalloc(4 * seq.size)
        d_nv = dmalloc(4 * n) if mode == "normal" else 0
        d_tl = dmalloc(4 * n) if mode == "trim" else 0
        d_mk = dmalloc(seq.size) if mode == "mask" else 0
        if seq.size:
            ctx.h2d(d_seq, seq)
        ctx.h2d(d_off, off)
        st = ctx.db_query_reads_device(view, k, both, d_seq, seq.size, d_off, n, min(o["ci"], 0xFFFFFFFF), d_cnt, d_nv, d_tl, d_mk)
        res = np.zeros(seq.size if mode == "mask" else n, dtype=np.uint8 if mode == "mask" else np.uint32)  # the per-position counters stay on the device
        if res.size:
            ctx.d2h(res, d_nv or d_tl or d_mk)
    finally:
        for d in allocs:
            ctx.free(d)
    t = rec.text
    lit = t.size  # the combined source: the text, the helpers' own bytes, the masked sequences
    nl, nl_plus_nl, gt = (lit, lit + 1), (lit, lit + 3), (lit + 3, lit + 4)
    src = np.concatenate([t, _LIT, res if mode == "mask" else res[:0].astype(np.uint8)])
    hs, he = rec.header
    ss, se = rec.seq
    length = se - ss
    fq_out = o["out_fastq"]
    if mode == "normal":
        if o["use_float"]:  # fastq_filter.cpp:119-120, float32; a read shorter than k is dropped
            n_win = np.maximum(length - k + 1, 0)
            lo, hi = (o["f_ci"] * n_win.astype(np.float32)).astype(np.uint32), (o["f_cx"] * n_win.astype(np.float32)).astype(np.uint32)
            keep = (res >= lo) & (res <= hi) & (length >= k)
        else:
            keep = (res >= o["ci"]) & (res <= o["cx"])
        if not o["in_fastq"]:
            segs = [(hs, rec.rec_end)]
        elif fq_out:  # the quality header's text is dropped
            segs = [(hs, rec.plus[0] + 1), (rec.plus[1], rec.rec_end)]
        else:
            segs = [gt, (hs + 1, rec.plus[0])]
    elif mode == "trim":
        keep = res > 0
        tl = res.astype(np.int64)
        head = [(hs, he)] if fq_out or not o["in_fastq"] else [gt, (hs + 1, he)]
        segs = head + [nl, (ss, ss + tl)] + ([nl_plus_nl, (rec.qual[0], rec.qual[0] + tl), nl] if fq_out else [nl])
    else:
        keep = np.ones(n, dtype=bool)
        ms = lit + _LIT.size + off[:-1].astype(np.int64)
        head = [(hs, he)] if fq_out or not o["in_fastq"] else [gt, (hs + 1, he)]
        segs = head + [nl, (ms, ms + length)] + ([nl_plus_nl, rec.qual, nl] if fq_out else [nl])
    sel = np.flatnonzero(keep)
    col = lambda v: np.full(sel.size, v, dtype=np.int64) if np.isscalar(v) else np.asarray(v, dtype=np.int64)[sel]  # noqa: E731
    starts = np.stack([col(a) for a, _ in segs], axis=1) if sel.size else np.zeros((0, len(segs)), dtype=np.int64)
    ends = np.stack([col(b) for _, b in segs], axis=1) if sel.size else starts
    return readsio.gather(src, starts, ends), n, int(sel.size), st


def filter_reads(argv, ctx=None) -> dict:
    """Runs the command line; returns dict(n_reads, n_written, and the summed tallies of kmc_hip_db_query_reads_device)."""
    o = parse_filter(argv)
    try:
        db = _read_input(o["db"])
    except (dbio.DbFormatError, OSError) as e:
        raise UsageError(str(e))
    if db.counter_size == 0:
        raise UsageError(f"{o['db']}: counter size 0 (a k-mer set without counters) is not supported")
    # CKMCFile::SetMinCount / SetMaxCount (kmc_file.cpp:664-698): a bound outside the database's own is ignored; the upper one is taken as 32 bits
    ci, cx = db.min_count, db.max_count
    if db.min_count <= o["db_ci"] <= cx:
        ci = o["db_ci"]
    if db.max_count >= (o["db_cx"] & 0xFFFFFFFF) >= ci:
        cx = o["db_cx"] & 0xFFFFFFFF
    part_bytes = max(1, int(float(os.environ.get("KMC_HIP_FILTER_PART_MB", "64")) * (1 << 20)))
    own = ctx is None
    if own:
        ctx = capi.Context((0,))
    dev = None
    total = dict(n_reads=0, n_written=0, **dict.fromkeys(capi.DBQ_STATS, 0))
    try:
        dev = _DeviceDb(ctx, db)
        view = dev.view(ci, cx)
        with open(o["out"], "wb") as out:
            for path in o["inputs"]:
                parts = readsio.parts(path, o["in_fastq"], part_bytes, ctx)
                while True:
                    try:
                        text = next(parts, None)  # a BGZF input is inflated on the device; what breaks in it is named here
                        if text is None:
                            break
                        data, n_in, n_out, st = _filter_part(ctx, view, db.kmer_len, db.both_strands, o, text)
                    except readsio.FormatError as e:
                        raise UsageError(f"{path}: {e}")
                    out.write(data.tobytes())
                    total["n_reads"] += n_in
                    total["n_written"] += n_out
                    for key in capi.DBQ_STATS:
                        total[key] += st[key]
    finally:
        if dev:
            dev.free()
        if own:
            ctx.close()
    return total


TRANSFORM_USAGE = """usage: python -m kmc_amd.tools transform <db> [-ci<v> -cx<v>] <oper> [-s] <out> [-ci<v> -cx<v> -cs<v> -okmc] [<oper> ...]
  <db>     a KMC database or a KFF file (KFF is read, not written); -ci / -cx: k-mers with a counter outside [ci, cx] are absent for every output (default: the database's own cutoffs)
  <oper>   sort | reduce | compact | set_counts <value>  write a KMC database <out> (-ci -cx: drop counters outside; -cs: clamp; compact stores counter 1)
           histogram  writes `counter<TAB>k-mers` for every counter in [-ci, -cx] (default -cx: the smallest of the database's, 10000 and what its counter bytes hold)
           dump [-s]  writes `k-mer<TAB>counter` per k-mer; -s, or any database output on the command line: in ascending k-mer order, otherwise in the input's order
  any number of <oper> ... <out> groups; the input is read once"""
TRANSFORM_DB_OPS = ("sort", "reduce", "compact", "set_counts")
HISTOGRAM_MAX_COUNTER_DEFAULT = 10000  # kmc_tools/defs.h
HISTOGRAM_MAX_BINS = 1 << 28
U32_MAX = 0xFFFFFFFF


def _num1(arg: str, name: str) -> int:
    """parameters_parser.cpp:16-25 replace_zero: a value of 0 is taken as 1"""
    return max(_num(arg, name), 1)


def parse_transform(argv):
    """-> ((path, ci, cx), [dict(op, path, sorted, ci, cx, cs, value)]); ci / cx / cs None = not given (parameters_parser.cpp:228-270,272-453)"""
    if not argv or argv[0].startswith("-"):
        raise UsageError("transform needs an input database\n" + TRANSFORM_USAGE)
    path, ci, cx = argv[0], None, None
    pos = 1
    while pos < len(argv) and argv[pos].startswith("-"):
        if argv[pos].startswith("-ci"):
            ci = _num1(argv[pos], "-ci")
        elif argv[pos].startswith("-cx"):
            cx = _num1(argv[pos], "-cx")
        else:
            raise UsageError(f"unknown input option {argv[pos]}")
        pos += 1
    outputs = []
    while pos < len(argv):
        op = argv[pos]
        if op not in TRANSFORM_DB_OPS + ("histogram", "dump"):
            raise UsageError(f"unknown operation: {op} (one of sort, reduce, compact, histogram, dump, set_counts)")
        o = dict(op=op, path=None, sorted=False, ci=None, cx=None, cs=None, value=0)
        pos += 1
        if op == "set_counts":
            if pos >= len(argv):
                raise UsageError("set_counts operation requires count value")
            if not argv[pos].isdigit():
                raise UsageError(f"Count value expected, but {argv[pos]} found")
            o["value"] = int(argv[pos])
            if o["value"] > U32_MAX:
                raise UsageError(f"set_counts: counter values up to {U32_MAX} are supported")
            pos += 1
        while pos < len(argv) and argv[pos].startswith("-"):
            if argv[pos] != "-s":
                raise UsageError(f"unknown operation parameter: {argv[pos]}")
            if op != "dump":
                raise UsageError("-s parameter allowed only for dump operation")
            o["sorted"] = True
            pos += 1
        if pos >= len(argv):
            raise UsageError(f"Output path missed ({op})")
        o["path"] = argv[pos]
        pos += 1
        while pos < len(argv) and argv[pos].startswith("-"):
            a = argv[pos]
            if a.startswith("-ci"):
                o["ci"] = _num1(a, "-ci")
            elif a.startswith("-cx"):
                o["cx"] = _num1(a, "-cx")
            elif a.startswith("-cs"):
                o["cs"] = _num1(a, "-cs")
            elif a.startswith("-o"):
                if op not in TRANSFORM_DB_OPS:
                    raise UsageError("-o parameter allowed only for compact, reduce, set_counts and sort operations")
                if a[2:] != "kmc":
                    raise UsageError(f"{a}: KFF output is not written, only KMC databases")
            else:
                raise UsageError(f"Unknown parameter: {a}")
            pos += 1
        outputs.append(o)
    if not outputs:
        raise UsageError("transform needs at least one <oper> <out>\n" + TRANSFORM_USAGE)
    return (path, ci, cx), outputs


def resolve_transform(outputs, db: dbio.Database, in_ci: int, in_cx: int) -> list:
    """The defaults of parameters_parser.cpp:437-450,867-892 -> per output dict(op, path, ci, cx, cs, value, cs_bytes (database outputs))."""
    full = (1 << (8 * db.counter_size)) - 1
    res = []
    for o in outputs:
        r = dict(op=o["op"], path=o["path"], value=o["value"])
        if o["op"] == "set_counts":  # the three options are ignored; a value of 0 sets nothing (kmc1_db_writer.h:378)
            r.update(ci=1, cx=U32_MAX, cs=U32_MAX)
        else:
            r["ci"] = o["ci"] or in_ci
            r["cx"] = o["cx"] or (min(db.max_count, HISTOGRAM_MAX_COUNTER_DEFAULT, full) if o["op"] == "histogram" else in_cx)
            r["cs"] = 1 if o["op"] == "compact" else (o["cs"] or full)
        if o["op"] in TRANSFORM_DB_OPS:
            r["cs_bytes"] = dbio.byte_log(r["value"]) if r["value"] else min(dbio.byte_log(r["cs"]), dbio.byte_log(r["cx"]))  # kmc1_db_writer.h:154-156
        res.append(r)
    return res


def _transform_database(ctx, dev, view, db, r, fmt="kmc1") -> dict:
    k = db.kmer_len
    p_out = dbio.best_lut_prefix_len(k, db.total_kmers)  # kmc1_db_writer.h:425-456, over the input header's total; a KFF output does not show it
    rb = (k - p_out) // 4 + r["cs_bytes"]
    d_out, d_lut = ctx.malloc(dev.n * rb + 256), ctx.malloc(8 << (2 * p_out))
    try:
        n, st = ctx.db_reduce_device(k, view, r["ci"], r["cx"], min(r["cs"], U32_MAX), r["value"], p_out, d_out, dev.n * rb, d_lut)
        _write_body(ctx, fmt, r["path"], k, capi.DbView(d_out, n, d_lut, p_out, r["cs_bytes"], r["ci"], r["cx"]), r["ci"], r["cx"], db.both_strands, mode=db.mode)
    finally:
        ctx.free(d_out)
        ctx.free(d_lut)
    return st


def _transform_histogram(ctx, dev, view, db, r) -> dict:
    ci, cx = r["ci"], min(r["cx"], U32_MAX)
    if cx < ci:  # histogram_writer.h:45: no line
        open(r["path"], "wb").close()
        return dict.fromkeys(capi.DBH_STATS, 0)
    n_bins = cx - ci + 1
    d_hist = ctx.malloc(8 * n_bins + 256)
    try:
        st = ctx.db_histogram_device(db.kmer_len, view, dev.n_seg, ci, cx, d_hist)
        hist = np.zeros(n_bins, dtype=np.uint64)
        ctx.d2h(hist, d_hist)
    finally:
        ctx.free(d_hist)
    with open(r["path"], "wb") as f:  # histogram_writer.h:45-48
        for i0 in range(0, n_bins, 1 << 16):
            f.write("".join(f"{ci + i0 + i}\t{c}\n" for i, c in enumerate(hist[i0:i0 + (1 << 16)].tolist())).encode())
    return st


def _transform_dump(ctx, dev, view, db, r) -> dict:
    k = db.kmer_len
    part_bytes = max(1, int(float(os.environ.get("KMC_HIP_DUMP_PART_MB", "64")) * (1 << 20)))
    part = max(1, part_bytes // (k + 12))  # records of a part: a record is at most k + 12 bytes of text
    cap = min(part, max(dev.n, 1)) * (k + 12)
    total = dict.fromkeys(capi.DBT_STATS, 0)
    total["n_bytes"] = 0
    d_text = ctx.malloc(cap + 256)
    try:
        with open(r["path"], "wb") as f:
            for first in range(0, dev.n, part):
                n_bytes, st = ctx.db_dump_device(k, view, dev.n_seg, first, min(part, dev.n - first), r["ci"], r["cx"], min(r["cs"], U32_MAX), d_text, cap)
                if n_bytes:
                    text = np.zeros(n_bytes, dtype=np.uint8)
                    ctx.d2h(text, d_text)
                    f.write(text.tobytes())
                total["n_bytes"] += n_bytes
                for key in capi.DBT_STATS:
                    total[key] += st[key]
    finally:
        ctx.free(d_text)
    return total


def transform(argv, ctx=None) -> list:
    """Runs the command line; returns per output that is written the dict of tallies of its device call(s) (a dump: summed over its parts, with n_bytes)."""
    (path, ci, cx), outputs = parse_transform(argv)
    try:
        db = _read_input(path)
    except (dbio.DbFormatError, OSError) as e:
        raise UsageError(str(e))
    if db.counter_size == 0:
        raise UsageError(f"{path}: counter size 0 (a k-mer set without counters) is not supported, as in kmc_tools")
    if not db.kmc2 and not isinstance(db, dbio.KffFile) and any(o["op"] == "sort" for o in outputs):  # kmc_tools.cpp:421-437: only a KMC1 input is sorted already
        print("Warning: input database is already sorted. Each sort operation will be omitted", file=sys.stderr)
        outputs = [o for o in outputs if o["op"] != "sort"]
        if not outputs:
            return []
    in_ci, in_cx = ci or db.min_count, cx or db.max_count
    res = resolve_transform(outputs, db, in_ci, in_cx)
    for r in res:
        if r["op"] == "histogram" and min(r["cx"], U32_MAX) - r["ci"] + 1 > HISTOGRAM_MAX_BINS:
            raise UsageError(f"histogram {r['path']}: a range of {min(r['cx'], U32_MAX) - r['ci'] + 1} counters; at most 2^28 = {HISTOGRAM_MAX_BINS} are written (give -cx)")
    # kmc_tools.cpp:440-465: one database output or one dump -s and every output sees the k-mers in ascending order
    need_order = any(o["op"] in TRANSFORM_DB_OPS or o["sorted"] for o in outputs)
    own = ctx is None
    if own:
        ctx = capi.Context((0,))
    dev = None
    results = []
    try:
        dev = _DeviceDb(ctx, db, order=need_order)
        view = dev.view(max(in_ci, 0), in_cx)
        for r in res:
            run = _transform_histogram if r["op"] == "histogram" else _transform_dump if r["op"] == "dump" else _transform_database
            results.append(run(ctx, dev, view, db, r))
    finally:
        if dev:
            dev.free()
        if own:
            ctx.close()
    return results


EXPORT_USAGE = """usage: python -m kmc_amd.tools export <db> [-ci<v> -cx<v>] <out> [-ci<v> -cx<v> -cs<v>] [--sections]
  writes <out>.kff, byte for byte the file of `kmc_tools transform <db> [-ci -cx] reduce <out> [-ci -cx -cs] -okff`: <db> (a KMC database as kmc or kmc_tools wrote
  it, or a KFF file of one or many sections) ordered where it is not, reduced by the bounds (defaults as for transform's reduce), framed as KFF records on the device
  and written as ONE ordered section.
  --sections  a KMC2 database (as `kmc` wrote it) only, and without any bounds: the body stays in file order and every bin that is not empty becomes one KFF section,
              under the input's own header values; no sort and no reduce. kmc_tools always orders, so this form has no reference twin: the file reads back (as an
              input of any mode here, or of kmc_tools) as the same k-mers and counters."""


def parse_export(argv):
    """-> ((path, ci, cx), dict(path, ci, cx, cs, sections)); ci / cx / cs None = not given"""
    if not argv or argv[0].startswith("-"):
        raise UsageError("export needs an input database\n" + EXPORT_USAGE)
    (path, ci, cx), pos = (argv[0], None, None), 1
    while pos < len(argv) and argv[pos].startswith("-") and argv[pos] != "--sections":
        if argv[pos].startswith("-ci"):
            ci = _num1(argv[pos], "-ci")
        elif argv[pos].startswith("-cx"):
            cx = _num1(argv[pos], "-cx")
        else:
            raise UsageError(f"unknown input option {argv[pos]}\n" + EXPORT_USAGE)
        pos += 1
    o = dict(path=None, ci=None, cx=None, cs=None, sections=False)
    for a in argv[pos:]:
        if a == "--sections":
            o["sections"] = True
        elif not a.startswith("-"):
            if o["path"] is not None:
                raise UsageError(f"export writes one output ({o['path']}, then {a})\n" + EXPORT_USAGE)
            o["path"] = a
        elif o["path"] is not None and a[:3] in ("-ci", "-cx", "-cs"):
            o[a[1:3]] = _num1(a, a[:3])
        else:
            raise UsageError(f"Unknown parameter: {a}\n" + EXPORT_USAGE)
    if o["path"] is None:
        raise UsageError("Output path missed (export)\n" + EXPORT_USAGE)
    if o["sections"] and any(v is not None for v in (ci, cx, o["ci"], o["cx"], o["cs"])):
        raise UsageError("export --sections copies the bins as they are: no -ci, -cx or -cs goes with it\n" + EXPORT_USAGE)
    return (path, ci, cx), o


def export(argv, ctx=None) -> dict:
    """Runs the command line; returns the dict of tallies of kmc_hip_db_reduce_device (--sections: n_written and n_sections)."""
    (path, ci, cx), o = parse_export(argv)
    try:
        db = _read_input(path)
    except (dbio.DbFormatError, OSError) as e:
        raise UsageError(str(e))
    if db.counter_size == 0:
        raise UsageError(f"{path}: counter size 0 (a k-mer set without counters) is not supported, as in kmc_tools")
    if o["sections"] and not db.kmc2:
        raise UsageError(f"{path}: export --sections takes a KMC2 database (as `kmc` wrote it); this input is " + ("a KFF file" if isinstance(db, dbio.KffFile) else "ordered already") + "\n" + EXPORT_USAGE)
    in_ci, in_cx = ci or db.min_count, cx or db.max_count
    r, = resolve_transform([dict(op="reduce", path=o["path"], ci=o["ci"], cx=o["cx"], cs=o["cs"], value=0)], db, in_ci, in_cx)
    own = ctx is None
    if own:
        ctx = capi.Context((0,))
    dev = None
    try:
        dev = _DeviceDb(ctx, db, order=not o["sections"])
        if not o["sections"]:
            return _transform_database(ctx, dev, dev.view(max(in_ci, 0), in_cx), db, r, fmt="kff")
        starts = db.raw_lut[:: 1 << (2 * db.lut_prefix_len)].astype(np.int64)  # the bins' first records, then the closing entry (n_bins x 4^p + 1 entries)
        secs = [(int(a), int(b - a)) for a, b in zip(starts[:-1], starts[1:]) if b > a] or [(0, 0)]
        _write_body(ctx, "kff", o["path"], db.kmer_len, dev.view(db.min_count, db.max_count), db.min_count, db.max_count, db.both_strands, n_seg=dev.n_seg, sections=secs)
        return dict(n_written=dev.n, n_sections=len(secs))
    finally:
        if dev:
            dev.free()
        if own:
            ctx.close()


COMPLEX_USAGE = """usage: python -m kmc_amd.tools complex <operations_definition_file>
  the file (kmc_tools' format):
    INPUT:
    <name> = <db> [-ci<v>] [-cx<v>]     one line per input, a KMC database or a KFF file; -ci / -cx: k-mers with a counter outside [ci, cx] count as absent
    ...
    OUTPUT:
    <out> = <expression>                 over the names: + union, * intersect (binds tighter), - kmers_subtract, ~ counters_subtract, parentheses; left to right.
                                         A counter mode min | max | diff | sum | left | right may stand directly behind + ~ * (defaults: + sum, * min, ~ diff)
    [OUTPUT_PARAMS:
    -ci<v> -cx<v> -cs<v> -okmc]          cutoffs and counter clamp of <out> (defaults: smallest input -ci, largest input -cx, largest counter the inputs can hold)
  At most 16 occurrences of inputs in the expression. Counters inside the expression are 32-bit and neither cut nor clamped; only <out> is."""
COMPLEX_KEYWORDS = ("min", "max", "diff", "sum", "left", "right")  # tokenizer.cpp:28-33, in the order they are tried
_TOKEN_PATTERNS = [(re.compile(p), t) for p, t in
                   [(r"\(", "("), (r"\)", ")"), (r"-", "-"), (r"~", "~"), (r"\+", "+"), (r"\*", "*")] + [(kw, kw) for kw in COMPLEX_KEYWORDS] + [(r"\w*", "var")]]
_EXPR_WHITESPACE = " \t\r\n\v\f"
_EXPR_OPS = {"+": ("union", "sum"), "-": ("kmers_subtract", "diff"), "~": ("counters_subtract", "diff"), "*": ("intersect", "min")}  # operator -> (operation, default mode)


def tokenize_expression(expr: str) -> list:
    """tokenizer.cpp:50-77 -> [(text, type)]: the patterns in the reference's order, each anchored at the front of what is left — so a keyword matches as a PREFIX
    (`minx` is `min`, `x`). Where no pattern consumes a character the reference loops for ever (`\\w*` matches the empty string); that is an error here."""
    tokens = []
    rest = expr.lstrip(_EXPR_WHITESPACE)
    while rest:
        for pat, typ in _TOKEN_PATTERNS:
            m = pat.match(rest)
            if m:
                break
        if not m.group(0):
            raise UsageError(f"wrong output format near: {rest}")
        tokens.append((m.group(0), typ))
        rest = rest[m.end():].lstrip(_EXPR_WHITESPACE)
    return tokens


def parse_expression(tokens: list, names: dict):
    """output_parser.h:94-208 -> the tree: ("in", index) | (operation, counter mode, left, right). expr -> term {(+|-|~) [mode] term}; term -> argument {* [mode] argument};
    argument -> name | ( expr ). Where the reference's argument() returns a null pointer that is dereferenced later, this raises."""
    if not tokens:
        raise UsageError("the output's expression is empty")
    pos = 0

    def cur():
        return tokens[pos] if pos < len(tokens) else ("", "end")

    def modifier(default):
        nonlocal pos
        if cur()[1] in COMPLEX_KEYWORDS:
            pos += 1
            return tokens[pos - 1][1]
        return default

    def argument():
        nonlocal pos
        text, typ = cur()
        if typ == "var":
            if text not in names:
                raise UsageError(f"variable {text} was not defined")
            pos += 1
            return ("in", names[text])
        if typ == "(":
            pos += 1
            res = expr()
            if cur()[1] != ")":
                raise UsageError(f"close parenthesis expected, but {cur()[0] or 'the end of the expression'} found")
            pos += 1
            return res
        raise UsageError(f"an input's name or '(' expected, but {text or 'the end of the expression'} found")

    def term():
        nonlocal pos
        left = argument()
        while cur()[1] == "*":
            pos += 1
            mode = modifier("min")
            left = ("intersect", mode, left, argument())
        return left

    def expr():
        nonlocal pos
        left = term()
        while cur()[1] in ("+", "-", "~"):
            op, default = _EXPR_OPS[cur()[1]]
            pos += 1
            mode = modifier(default) if op != "kmers_subtract" else default  # no modifier behind '-' (output_parser.h:192-195)
            left = (op, mode, left, term())
        return left

    tree = expr()
    if pos < len(tokens):
        raise UsageError(f"wrong symbol: {cur()[0]}")
    return tree


def expr_steps(tree) -> list:
    """the tree as the postfix program of kmc_hip_db_expr_device: [(kind, arg)]"""
    if tree[0] == "in":
        return [(capi.DB_EXPR_INPUT, tree[1])]
    return expr_steps(tree[2]) + expr_steps(tree[3]) + [(capi.DB_OPS[tree[0]], capi.DB_COUNTER_OPS[tree[1]])]


_INPUT_LINE = re.compile(r"^\s*([\w+-]*)\s*=\s*(.*)$", re.ASCII)  # parser.cpp:31-32
_OUTPUT_LINE = re.compile(r"^\s*(.*)\s*=\s*(.*)$", re.ASCII)


def parse_complex(text: str) -> dict:
    """The operations-definition file, split as kmc_tools/parser.cpp splits it -> dict(inputs [(name, path, ci, cx)], path, tree, ci, cx, cs); 0 = not given"""
    lines = iter([ln for ln in text.split("\n") if ln.strip(_EXPR_WHITESPACE)])  # nextLine: blank lines are skipped
    for ln in lines:
        if "INPUT:" in ln:
            break
    else:
        raise UsageError("'INPUT:' missing")
    ln = next(lines, None)
    if ln is None or "OUTPUT:" in ln:
        raise UsageError("None input was defined")
    inputs, names = [], {}
    while True:
        m = _INPUT_LINE.search(ln)
        if not m:
            raise UsageError(f"wrong line format: {ln}")
        name, words = m.group(1), m.group(2).split()
        if name in names:
            raise UsageError(f"Name redefinition({name})")
        if name in COMPLEX_KEYWORDS:
            raise UsageError(f"`{name}` is not valid name")
        if not words:
            raise UsageError(f"file name for {name} was not specified")
        ci = cx = 0
        for w in words[1:]:
            if w.startswith("-ci"):
                ci = _num(w, "-ci")
            elif w.startswith("-cx"):
                cx = _num(w, "-cx")
            else:
                raise UsageError(f"Unknow parameter {w} for variable {name}")
        names[name] = len(inputs)
        inputs.append((name, words[0], ci, cx))
        ln = next(lines, None)
        if ln is None:
            raise UsageError("'OUTPUT:' missing")
        if "OUTPUT:" in ln:
            break
    ln = next(lines, None)
    if ln is None or "OUTPUT_PARAMS:" in ln:
        raise UsageError("None output was defined")
    m = _OUTPUT_LINE.search(ln)
    if not m:
        raise UsageError(f"wrong line format: {ln}")
    path = m.group(1).rstrip(_EXPR_WHITESPACE)
    if not path:
        raise UsageError(f"wrong line format (output file name is not specified): {ln}")
    tree = parse_expression(tokenize_expression(m.group(2)), names)
    o = dict(inputs=inputs, path=path, tree=tree, ci=0, cx=0, cs=0)
    for ln in lines:
        if "OUTPUT_PARAMS:" not in ln:
            continue
        for w in (next(lines, None) or "").split():
            if w.startswith("-ci"):
                o["ci"] = _num(w, "-ci")
            elif w.startswith("-cx"):
                o["cx"] = _num(w, "-cx")
            elif w.startswith("-cs"):
                o["cs"] = _num(w, "-cs")
            elif w.startswith("-o"):
                if w[2:5] == "kff":
                    raise UsageError(f"{w}: KFF output is not written, only KMC databases")
                if w[2:5] != "kmc":
                    raise UsageError(f"Unknown output type: {w[2:]}")
            else:
                raise UsageError(f"Unknow parameter {w}")
        break
    return o


def _leaves(tree) -> list:
    return [tree[1]] if tree[0] == "in" else _leaves(tree[2]) + _leaves(tree[3])


def resolve_complex(o: dict, dbs: list) -> dict:
    """The defaults (parameters_parser.cpp:842-848, 893-916; kmc1_db_writer.h:425-455) over ALL defined inputs, used in the expression or not.
    dbs: objects with kmer_len, counter_size, min_count, max_count, total_kmers, both_strands -> dict(cuts, ci, cx, cs, cs_bytes, p_out, canonical)"""
    k = dbs[0].kmer_len
    for (name, path, _, _), db in zip(o["inputs"], dbs):
        if db.kmer_len != k:
            raise UsageError(f"the inputs have different k-mer lengths ({k} and {db.kmer_len})")
        if db.counter_size == 0:
            raise UsageError(f"{path}: counter size 0 (a k-mer set without counters) is not supported, as in kmc_tools")
    cuts = [(ci or db.min_count, cx or db.max_count) for (_, _, ci, cx), db in zip(o["inputs"], dbs)]
    ci, cx = o["ci"] or min(c[0] for c in cuts), o["cx"] or max(c[1] for c in cuts)
    cs = o["cs"] or (1 << (8 * max(db.counter_size for db in dbs))) - 1
    return dict(cuts=cuts, ci=ci, cx=cx, cs=cs, cs_bytes=min(dbio.byte_log(cs), dbio.byte_log(cx)), p_out=max(dbio.best_lut_prefix_len(k, db.total_kmers) for db in dbs),
                canonical=all(db.both_strands for db in dbs))


def _read_header(path: str) -> dbio.Database:
    """the header of <path>.kmc_pre alone (the fields dbio.read_database reads from it): what an input contributes that the expression does not name"""
    with open(path + ".kmc_pre", "rb") as f:
        f.seek(0, os.SEEK_END)
        size = f.tell()
        f.seek(max(size - 256, 0))
        tail = np.frombuffer(f.read(), dtype=np.uint8)
    if size < 16 or bytes(tail[-4:]) != b"KMCP" or int(tail[-8:-4].copy().view(np.uint32)[0]) + 8 > tail.size:
        raise dbio.DbFormatError(f"{path}.kmc_pre: no KMCP markers")
    header_offset = int(tail[-8:-4].copy().view(np.uint32)[0])
    kmc2 = int(tail[-12:-8].copy().view(np.uint32)[0]) == 0x200
    h = tail[tail.size - 8 - header_offset: tail.size - 8]
    u32 = lambda o: int(h[o:o + 4].copy().view(np.uint32)[0])  # noqa: E731
    o = 20 if kmc2 else 16
    return dbio.Database(u32(0), u32(4), u32(8), u32(12), u32(16) if kmc2 else 0, u32(o), (u32(o + 20) << 32) + u32(o + 4), int(h[o + 8:o + 16].copy().view(np.uint64)[0]),
                         int(h[o + 16]) != 1, kmc2)


def _tree_bound(tree, n) -> int:
    if tree[0] == "in":
        return n[tree[1]]
    lt, rt = _tree_bound(tree[2], n), _tree_bound(tree[3], n)
    return lt + rt if tree[0] == "union" else min(lt, rt) if tree[0] == "intersect" else lt


def complex(argv, ctx=None) -> dict:  # noqa: A001 (the mode's name)
    """Runs the operations-definition file argv[0]; returns the dict of tallies of kmc_hip_db_expr_device."""
    if len(argv) != 1 or argv[0].startswith("-"):
        raise UsageError(COMPLEX_USAGE)
    try:
        with open(argv[0]) as f:
            o = parse_complex(f.read())
    except OSError as e:
        raise UsageError(f"cannot open file: {argv[0]} ({e.strerror})")
    leaves = _leaves(o["tree"])
    if len(leaves) > capi.DB_EXPR_MAX_LEAVES:
        raise UsageError(f"the expression names inputs {len(leaves)} times; at most {capi.DB_EXPR_MAX_LEAVES} are evaluated")
    used = sorted(set(leaves))
    dbs = []
    for i, (_, path, _, _) in enumerate(o["inputs"]):
        try:
            kff = dbio.is_kff(path) and not os.path.exists(path + ".kmc_pre")
            dbs.append(_read_input(path) if i in used or kff else _read_header(path))  # a database that is defined but not used: its header only
        except (dbio.DbFormatError, OSError) as e:
            raise UsageError(str(e))
    r = resolve_complex(o, dbs)
    k = dbs[0].kmer_len
    own = ctx is None
    if own:
        ctx = capi.Context((0,))
    dev = {}
    try:
        for i in used:
            dev[i] = _DeviceDb(ctx, dbs[i])
        # the views of the inputs the expression names, and the program over those
        slot = {i: q for q, i in enumerate(used)}
        views = [dev[i].view(*r["cuts"][i]) for i in used]
        steps = [(kind, slot[arg] if kind == capi.DB_EXPR_INPUT else arg) for kind, arg in expr_steps(o["tree"])]
        rb = (k - r["p_out"]) // 4 + r["cs_bytes"]
        bound = _tree_bound(o["tree"], {i: dev[i].n for i in used})
        d_out, d_lut = ctx.malloc(bound * rb + 256), ctx.malloc(8 << (2 * r["p_out"]))
        try:
            n, st = ctx.db_expr_device(k, views, steps, capi.DbOp(0, 0, r["ci"], r["cs"], r["cx"], r["p_out"]), d_out, bound * rb, d_lut)
            _write_body(ctx, "kmc1", o["path"], k, capi.DbView(d_out, n, d_lut, r["p_out"], r["cs_bytes"], r["ci"], r["cx"]), r["ci"], r["cx"], r["canonical"], mode=dbs[0].mode)
        finally:
            ctx.free(d_out)
            ctx.free(d_lut)
    finally:
        for d in dev.values():
            d.free()
        if own:
            ctx.close()
    return st


COMPARE_USAGE = """usage: python -m kmc_amd.tools compare <db1> [-ci<v> -cx<v>] <db2> [-ci<v> -cx<v>]
  prints `DB Equals` (exit status 0) or `DB Differs` (1): the k-mers of each input whose counter lies in its [-ci, -cx] (default: the database's own cutoffs), walked in
  ascending order, must agree pair by pair in counter and k-mer; `one of input is not finished` in front where one input ends first"""
CHECK_USAGE = """usage: python -m kmc_amd.tools check <db> [-ci<v> -cx<v>] <kmer>
  prints the counter of <kmer> in <db>, 0 where it is absent or its counter is below -ci or NOT BELOW -cx (kmc_tools' rule for this mode); the k-mer is looked up as
  given, not its canonical form. A KFF file that does not hold it prints nothing"""
INFO_USAGE = """usage: python -m kmc_amd.tools info <db>
  prints the header of a KMC database, or the encoding, the scopes and the data sections of a KFF file, as kmc_tools does (headers only: no device is opened)"""


class RefError(UsageError):
    """an error kmc_tools itself reports: its own words on stderr, exit status 1"""

    def __init__(self, msg):
        SystemExit.__init__(self, msg)


def _input_desc(argv, pos):
    """parameters_parser.cpp:238-270 read_input_desc -> (path, ci, cx, pos); None = not given: up to two of -ci / -cx behind the name"""
    if pos >= len(argv):
        raise UsageError("Input database source missed")
    if argv[pos].startswith("-"):
        raise UsageError(f"Input database source required, but {argv[pos]}found")
    path, ci, cx = argv[pos], None, None
    pos += 1
    for _ in range(2):
        if pos >= len(argv) or not argv[pos].startswith("-"):
            break
        if argv[pos].startswith("-ci"):
            ci = _num1(argv[pos], "-ci")
        elif argv[pos].startswith("-cx"):
            cx = _num1(argv[pos], "-cx")
        else:
            raise UsageError(f"Unknow parameter: {argv[pos]}")
        pos += 1
    return path, ci, cx, pos


def _validated_inputs(descs):
    """parameters_parser.cpp:752-795,842-848 validate_input_dbs -> [(db, ci, cx)] with the cutoffs' defaults from the headers"""
    dbs = []
    for path, _, _ in descs:
        try:
            dbs.append(_read_input(path))
        except (dbio.DbFormatError, OSError) as e:
            raise UsageError(str(e))
    if dbs[0].mode == 1:
        raise UsageError("quality counters are not supported in kmc tools")
    for (path, _, _), db in zip(descs[1:], dbs[1:]):
        if db.mode != dbs[0].mode:
            raise UsageError("quality/direct based counters conflict!")
        if db.kmer_len != dbs[0].kmer_len:
            raise UsageError(f"Database {descs[0][0]} contains {dbs[0].kmer_len}-mers, but database {path} contains {db.kmer_len}-mers")
    for (path, _, _), db in zip(descs, dbs):
        if db.counter_size == 0:
            raise UsageError(f"{path}: counter size 0 (a k-mer set without counters) is not supported, as in kmc_tools")
    return [(db, ci or db.min_count, cx or db.max_count) for (_, ci, cx), db in zip(descs, dbs)]


def parse_compare(argv):
    """-> [(path, ci, cx)] x 2; None = not given (parameters_parser.cpp:709-713)"""
    if not argv:
        raise UsageError(COMPARE_USAGE)
    a = _input_desc(argv, 0)
    b = _input_desc(argv, a[3])
    if b[3] < len(argv):
        raise UsageError(f"Unknow parameter: {argv[b[3]]}\n" + COMPARE_USAGE)
    return [a[:3], b[:3]]


def _dump_one(ctx, dev, k, record) -> str:
    """the k-mer of one record of a body as text: a one-record kmc_hip_db_dump_device with the cutoffs wide open"""
    d_text = ctx.malloc(k + 12 + 256)
    try:
        n_bytes, _ = ctx.db_dump_device(k, dev.view(0, U32_MAX), dev.n_seg, record, 1, 1, U32_MAX, U32_MAX, d_text, k + 12)
        text = np.zeros(n_bytes, dtype=np.uint8)
        if n_bytes:
            ctx.d2h(text, d_text)
    finally:
        ctx.free(d_text)
    return text.tobytes().decode().split("\t")[0]


def compare(argv, ctx=None) -> dict:
    """Runs the command line; returns result[] of kmc_hip_db_compare_device as a dict (capi.DBC_RESULT; kind by its name in capi.DBC_KINDS) and, where the inputs
    differ, kmer_a / kmer_b: the text of the two k-mers at the first difference (None for an input that ended)."""
    ins = _validated_inputs(parse_compare(argv))
    k = ins[0][0].kmer_len
    own = ctx is None
    if own:
        ctx = capi.Context((0,))
    dev = []
    try:
        dev = [_DeviceDb(ctx, db, order=True) for db, _, _ in ins]
        res = ctx.db_compare_device(k, *(d.view(ci, cx) for d, (_, ci, cx) in zip(dev, ins)))
        res["kind"] = capi.DBC_KINDS[res["kind"]]
        if res["kind"] != "equal":
            for q, d in zip("ab", dev):
                res["kmer_" + q] = _dump_one(ctx, d, k, res["record_" + q]) if res["record_" + q] < d.n else None
    finally:
        for d in dev:
            d.free()
        if own:
            ctx.close()
    return res


def compare_report(res: dict) -> str:
    """what kmc_tools prints (operations.h:288, kmc_tools.cpp:518-527)"""
    if res["kind"] == "equal":
        return "DB Equals\n"
    return ("one of input is not finished\n" if res["kind"] in ("a_ended", "b_ended") else "") + "DB Differs\n"


CHECK_PART_KMERS_ENV = "KMC_HIP_CHECK_PART_MB"
_KMER_SYMBOLS = frozenset(b"ACGTacgt")


def parse_check(argv):
    """-> ((path, ci, cx), kmer) (parameters_parser.cpp:704-708,228-236)"""
    if not argv:
        raise UsageError(CHECK_USAGE)
    path, ci, cx, pos = _input_desc(argv, 0)
    if pos >= len(argv):
        raise UsageError("check operation require k-mer to check")
    return (path, ci, cx), argv[pos]


def _check_counters(db, ci, cx, kmers, ctx) -> np.ndarray:
    """-> per k-mer the counter the database holds for it as given (0: none), after the rule of check_kmer.h:48,79: present while (uint32)(counter - ci) <
    (uint32)(cx - ci) — a counter EQUAL to cx is absent, unlike in every other mode"""
    k = db.kmer_len
    lines = []
    for kmer in kmers:
        b = kmer.encode("latin-1") if isinstance(kmer, str) else bytes(kmer)
        if len(b) != k:  # check_kmer.h:196-200
            raise RefError("Error: invalid k-mer length")
        lines.append(b)
    for b in lines:
        if not _KMER_SYMBOLS.issuperset(b):  # check_kmer.h:216-233
            raise RefError("Error: invalid k-mer format")
    out = np.zeros(len(lines), dtype=np.uint32)
    if not lines:
        return out
    part = max(1, int(float(os.environ.get(CHECK_PART_KMERS_ENV, "64")) * (1 << 20)) // (k + 1))  # k-mers of a part: a line is k + 1 bytes
    own = ctx is None
    if own:
        ctx = capi.Context((0,))
    dev = None
    try:
        dev = _DeviceDb(ctx, db, order=True)  # one upload of the database
        view = dev.view(0, U32_MAX)  # every record present: the rule is applied below
        for first in range(0, len(lines), part):
            seq = np.frombuffer(b"".join(ln + b"\n" for ln in lines[first:first + part]), dtype=np.uint8)
            d_seq, d_cnt = ctx.malloc(seq.size + 256), ctx.malloc(4 * seq.size + 256)
            try:
                ctx.h2d(d_seq, seq)
                ctx.db_query_reads_device(view, k, False, d_seq, seq.size, 0, 0, 0, d_cnt)
                cnt = np.zeros(seq.size, dtype=np.uint32)
                ctx.d2h(cnt, d_cnt)
            finally:
                ctx.free(d_seq)
                ctx.free(d_cnt)
            out[first:first + part] = cnt[::k + 1]  # the window that starts a line is the line's k-mer
    finally:
        if dev:
            dev.free()
        if own:
            ctx.close()
    present = ((out.astype(np.int64) - ci) & U32_MAX) < ((cx - ci) & U32_MAX)
    return np.where(present, out, 0).astype(np.uint32)


def check_kmers(db_path, kmers, ci=None, cx=None, ctx=None) -> np.ndarray:
    """The batch form of `check`: the counters of `kmers` (text of k symbols each) in the database at db_path, uint32, 0 where `check` prints 0 or nothing. The
    database goes up once; the k-mers go through in parts as lines of a reads buffer of kmc_hip_db_query_reads_device."""
    (db, ci, cx), = _validated_inputs([(db_path, ci, cx)])
    return _check_counters(db, ci, cx, list(kmers), ctx)


def check(argv, ctx=None) -> str:
    """Runs the command line; returns what kmc_tools prints: the counter and a line end — for a KFF file that does not hold the k-mer, nothing (check_kmer.h:375-401)"""
    desc, kmer = parse_check(argv)
    (db, ci, cx), = _validated_inputs([desc])
    c = int(_check_counters(db, ci, cx, [kmer], ctx)[0])
    return "" if isinstance(db, dbio.KffFile) and c == 0 else f"{c}\n"


def info(argv) -> tuple:
    """Runs the command line; returns (stdout text, stderr text) of CTools::info() (kmc_tools.cpp:139-224). Headers only: no device."""
    if not argv:
        raise UsageError(INFO_USAGE)
    path, _, _, _ = _input_desc(argv, 0)
    try:
        if dbio.is_kff(path) and not os.path.exists(path + ".kmc_pre"):
            return _info_kff(dbio.read_kff(path))
        h = _read_header(path)
        size = os.path.getsize(path + ".kmc_pre")
        with open(path + ".kmc_pre", "rb") as f:
            f.seek(size - 8)
            header_offset = int.from_bytes(f.read(4), "little")
    except (dbio.DbFormatError, OSError) as e:
        raise UsageError(str(e))
    if h.mode == 1:
        raise UsageError("quality counters are not supported in kmc tools")
    n_bins = 0
    if h.kmc2:  # kmer_file_header.cpp:96-101, in its 32-bit arithmetic
        single_lut, map_size = ((1 << (2 * h.lut_prefix_len)) * 8) & U32_MAX, (((1 << (2 * h.signature_len)) + 1) * 4) & U32_MAX
        n_bins = ((size - 8 - 12 - header_offset - map_size) // single_lut) & U32_MAX
    rows = [("k", h.kmer_len), ("total k-mers", h.total_kmers), ("cutoff max", h.max_count), ("cutoff min", h.min_count), ("counter size", f"{h.counter_size} bytes"),
            ("mode", "quality-aware counters" if h.mode else "occurrence counters"), ("both strands", "yes" if h.both_strands else "no"),
            ("database format", "KMC2.x" if h.kmc2 else "KMC1.x"), ("signature length", h.signature_len), ("number of bins", n_bins), ("lut_prefix_len", h.lut_prefix_len)]
    return "".join("%-18s:  %s\n" % r for r in rows), ""


def _info_kff(kff) -> tuple:
    """kmc_tools.cpp:157-216. A raw section has no minimizer bytes: its `minimizer (HEX)` line is empty (and std::hex, set inside the loop over them, never is)"""
    yes = lambda v: "yes" if v else "no"  # noqa: E731
    out = ["This is KFF file, summary:\n", f"canonical         :  {yes(kff.both_strands)}\n", f"all k-mers unique :  {yes(kff.all_unique)}\n", "symbols encoding:\n"]
    out += [f"\t{s}: {(kff.encoding >> sh) & 3}\n" for s, sh in zip("ACGT", (6, 4, 2, 0))]
    err = []
    for variables, sections in kff.scopes:
        out += [f"k             :  {variables['k']}\n", f"data_size     :  {variables['data_size']}\n", f"max           :  {variables['max']}\n"]
        if "m" in variables:
            out.append(f"m             :  {variables['m']}\n")
        err.append("footer values:\n")
        err += [f"\t{name}      :  {value}\n" for name, value in sorted(kff.footer.items())]
        out.append("Data sections:\n")
        for start, n in sections:
            out += ["\ttype            :  raw\n", f"\tdata_start      :  {start}\n", f"\tnb_blocks       :  {n}\n", "\tminimizer (HEX) :  \n"]
        out.append(f"tot_nb_blocks :  {sum(n for _, n in sections)}\n")
    return "".join(out), "".join(err)


COUNT_USAGE = """usage: python -m kmc_amd.tools count [options] <input_file | @file_of_inputs> <out> [<working_dir>]
  the argument order of `kmc`, so a kmc command line carries over. Read: -k<len> (25; 14..224) -ci<v> (2) -cx<v> (1e9) -cs<v> (255) -b -fa | -fq (default) | -fm -hc
  -p<signature_len> (min(9, k); 5..11) -n<bins> (512; at most 2048). Accepted and ignored (they size the reference's host pipeline): -t* -m* -r -sf* -sp* -sr* -v and
  <working_dir>. Everything else is refused. Writes <out>.kmc_pre / .kmc_suf as `kmc` followed by `kmc_tools transform <db> sort <out>` does; with
  KMC_HIP_COUNT_OUT=kff in the environment <out>.kff instead, as `kmc -okff` followed by `kmc_tools transform <out>.kff reduce <out2> -okff` does.
  A bgzipped input (BGZF: what `bgzip` writes) is recognised by its content and inflated on the device; plain gzip is inflated on the host. With KMC_HIP_COUNT_IN=bam
  in the environment the inputs are BAM files (what `kmc -fbam` reads); -fa / -fq / -fm are then refused."""
COUNT_PART_BYTES = 32 << 20
COUNT_MAP_MULTIPLIER = 0x9E3779B1
_COUNT_REFUSED = {"-okff": "KFF output", "-e": "the k-mer number estimation alone", "--opt-out-size": "the output size optimisation", "-fbam": "BAM input is chosen with "
                  "KMC_HIP_COUNT_IN=bam in the environment or input_format=\"bam\" of tools.count / tools.count_small, not with this option yet", "-fkmc": "KMC-database input", "-sm": "strict memory mode", "-j": "the JSON summary", "-w": "a run without output"}


def _count_options(argv, verb: str, usage: str):
    """the option loop of `count` and `count-small` (kmc's own grammar) -> (dict(k, ci, cx, cs, both, file_type, hc, m, n_bins), positional arguments)"""
    o = dict(k=25, ci=2, cx=10**9, cs=255, both=True, file_type=1, hc=False, m=None, n_bins=512)
    pos = []
    for a in argv:
        if not a.startswith("-") or a == "-":
            pos.append(a)
        elif a.startswith(("-t", "-m", "-sf", "-sp", "-sr")) and not a.startswith("-sm") or a in ("-r", "-v"):
            continue  # threads, memory, RAM-only mode, the splitters / readers / sorters, verbosity: they size the reference's host pipeline
        elif a.startswith("-ci"):
            o["ci"] = _num(a, a[:3])
        elif a.startswith("-cx"):
            o["cx"] = _num(a, a[:3])
        elif a.startswith("-cs"):
            o["cs"] = _num(a, a[:3])
        elif a.startswith("-k"):
            o["k"] = _num(a, a[:2])
        elif a.startswith("-p"):
            o["m"] = _num(a, a[:2])
        elif a.startswith("-n"):
            o["n_bins"] = _num(a, a[:2])
        elif a == "-b":
            o["both"] = False
        elif a == "-hc":
            o["hc"] = True
        elif a in ("-fa", "-fq", "-fm"):
            o["file_type"] = {"-fa": 0, "-fq": 1, "-fm": 2}[a]
        else:
            why = next((w for pre, w in _COUNT_REFUSED.items() if a.startswith(pre)), None)
            raise UsageError(f"{verb}: option {a} is not read" + (f" ({why})" if why else "") + "\n" + usage)
    return o, pos


def _count_inputs(o: dict, pos: list) -> dict:
    """<input | @list> <out> of the command line into o["inputs"], o["out"]"""
    if pos[0].startswith("@"):
        try:
            with open(pos[0][1:]) as f:
                o["inputs"] = [ln.strip() for ln in f if ln.strip()]
        except OSError as e:
            raise UsageError(f"cannot open file: {pos[0][1:]} ({e.strerror})")
    else:
        o["inputs"] = [pos[0]]
    o["out"] = pos[1]
    return o


def parse_count(argv) -> dict:
    """-> dict(k, ci, cx, cs, both, file_type (0 FASTA, 1 FASTQ, 2 multi-line FASTA), hc, m, n_bins, inputs, out)"""
    o, pos = _count_options(argv, "count", COUNT_USAGE)
    if len(pos) not in (2, 3):
        raise UsageError(COUNT_USAGE)
    k = o["k"]
    if k < 14:
        raise UsageError(f"count: -k{k}: k <= 13 is counted without bins, by the small-k entries of the library (kmc_hip_smallk_open / _part / _read); this front end takes k 14..224 (`count-small` is the verb for k <= 13)")
    if k > 224:
        raise UsageError(f"count: -k{k}: at most 224 (the ordered database's record width)")
    if o["m"] is None:
        o["m"] = min(9, k)
    if not 5 <= o["m"] <= 11:
        raise UsageError(f"count: -p{o['m']}: the signature length is 5..11")
    if not 1 <= o["n_bins"] <= 2048:
        raise UsageError(f"count: -n{o['n_bins']}: 1..2048 bins")
    if o["ci"] < 1 or o["cs"] < 1 or o["cx"] < o["ci"]:
        raise UsageError("count: -ci and -cs are at least 1, -cx at least -ci")
    return _count_inputs(o, pos)


def count_signature_map(signature_len: int, n_bins: int, multiplier: int = COUNT_MAP_MULTIPLIER) -> np.ndarray:
    """The signature -> bin map of `count`, int32[4^m + 1] (the last entry is the special signature's): bin = ((sig * multiplier mod 2^32) >> 8) % n_bins, a fixed
    pseudo-random spread. It does not reproduce CSignatureMapper's balancing from stage-0 statistics; the database does not depend on the map (all occurrences of a
    k-mer share one signature), only the balance of the bins does, which the run reports."""
    sig = np.arange((1 << (2 * signature_len)) + 1, dtype=np.uint64)
    return ((((sig * np.uint64(multiplier)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)) % np.uint64(n_bins)).astype(np.int32)


COUNT_MAP_MIN_BINS = 64  # the reference's own minimum of -n (kmc_CLI/kmc.cpp); below it CSignatureMapper::Init's arithmetic breaks (n_bins 2: it assigns bin 2)


def balanced_signature_map(stats: np.ndarray, signature_len: int, n_bins: int, allowed: np.ndarray = None) -> np.ndarray:
    """CSignatureMapper::Init (s_mapper.h:141-235) restated: the signature -> bin map, int32[4^m + 1], from the stage-0 statistics (uint32[4^m + 1]: k-mer windows
    per signature). Only allowed signatures take part, each with stats + 1000, in descending order (ties: ascending signature; the reference's std::sort leaves
    ties unspecified, so its exact map is not reproduced). While more signatures are left than bins: one above the running mean (what is left / the bins that are
    left) gets a bin alone, otherwise a bin takes, in that order, every signature that still fits under 1.1 x the mean. The rest get a bin each, the special
    signature (entry 4^m) the bin behind the last one used; entries that are not allowed stay -1. allowed: bool[4^m + 1], by default the library's own
    (capi.allowed_signatures). n_bins >= COUNT_MAP_MIN_BINS."""
    size = (1 << (2 * signature_len)) + 1
    stats = np.asarray(stats)
    if stats.size != size:
        raise ValueError(f"balanced_signature_map: {stats.size} statistics for signature length {signature_len}")
    if n_bins < COUNT_MAP_MIN_BINS:
        raise ValueError(f"balanced_signature_map: {n_bins} bins; the reference's mapper needs {COUNT_MAP_MIN_BINS} at least")
    if allowed is None:
        allowed = capi.allowed_signatures(signature_len)
    out = np.full(size, -1, dtype=np.int32)
    sig = np.flatnonzero(np.asarray(allowed, dtype=bool)[:size - 1])
    w = stats[sig].astype(np.float64) + 1000.0
    order = np.argsort(-w, kind="stable")  # descending weight, ascending signature among equals
    sig, w = sig[order], w[order]
    total = float(w.sum())
    mean = total / n_bins
    max_bin = 1.1 * mean
    n, max_bins, bin_no = n_bins - 1, n_bins - 1, 0  # one bin is kept for the special signature
    while sig.size > n:
        if w[0] > mean:
            out[sig[0]] = bin_no
            bin_no += 1
            total -= float(w[0])
            sig, w = sig[1:], w[1:]
        else:
            # first fit over the descending list: a signature is taken iff what the bin holds + its weight stays below max_bin. Taken in runs: from the first one
            # that fits (the list descends: a binary search), as many consecutive ones as fit (their prefix sums: weights are whole numbers, the sums exact)
            pre = np.concatenate([[0.0], np.cumsum(w)])
            desc = -w
            take = np.zeros(sig.size, dtype=bool)
            tmp, pos = 0.0, 0
            while pos < sig.size:
                j = max(pos, int(np.searchsorted(desc, -(max_bin - tmp), side="right")))  # the first w[j] < max_bin - tmp
                if j >= sig.size:
                    break
                end = int(np.searchsorted(pre, max_bin - tmp + pre[j], side="left")) - 1  # the largest end with tmp + (pre[end] - pre[j]) < max_bin
                take[j:end] = True
                tmp += float(pre[end] - pre[j])
                pos = end
            out[sig[take]] = bin_no
            bin_no += 1
            total -= tmp
            sig, w = sig[~take], w[~take]
        n -= 1
        mean = total / (max_bins - bin_no) if max_bins > bin_no else 0.0
        max_bin = 1.1 * mean
    out[sig] = bin_no + np.arange(sig.size, dtype=np.int32)
    out[size - 1] = bin_no + sig.size
    if int(out[size - 1]) >= n_bins:  # the reference would write bin n_bins here (groups that stay far below their bound); not met with real statistics
        raise ValueError(f"balanced_signature_map: the statistics need more than {n_bins} bins")
    return out


def _input_format(verb: str, input_format, argv) -> bool:
    """is the input BAM? input_format: None / "reads" (what the options say) or "bam", which the file-type options contradict"""
    if input_format not in (None, "reads", "bam"):
        raise ValueError(f'{verb}: input_format is "reads" or "bam", not {input_format!r}')
    if input_format == "bam" and any(a in ("-fa", "-fq", "-fm") for a in argv):
        raise UsageError(f"{verb}: BAM input and {next(a for a in argv if a in ('-fa', '-fq', '-fm'))} contradict each other")
    return input_format == "bam"


def _count_parts(o: dict, path: str, part_bytes: int, ctx):
    """the parts of one input file as the session takes them under o["file_type"]; a BGZF file is inflated on the device"""
    if o["file_type"] == capi.SPLIT_FILE_BAM:
        return readsio.bam_parts(path, part_bytes, ctx)
    return multiline_parts(path, part_bytes, ctx) if o["file_type"] == 2 else readsio.parts(path, o["file_type"] == 1, part_bytes, ctx)


def count_stats_sample(ctx, o: dict, part_bytes: int) -> np.ndarray:
    """stage 0 of `count`: the first part of every input file through a capi.SigStats accumulator -> the statistics, uint32[4^m + 1]"""
    acc = capi.SigStats(ctx, o["k"], o["m"])
    try:
        for path in o["inputs"]:
            try:
                part = next(iter(_count_parts(o, path, part_bytes, ctx)), None)
            except OSError as e:
                raise UsageError(f"cannot open file: {path} ({e.strerror})")
            except readsio.FormatError as e:
                raise UsageError(f"count: {path}: {e}")
            if part is None:
                continue
            try:
                acc.part(part, file_type=o["file_type"], flags=capi.SPLIT_HOMOPOLYMER if o["hc"] else 0)
            except capi.KmcHipError as e:
                if e.code == capi.UNCOVERED:
                    raise UsageError(f"count: {path}, part 0: {e}")
                raise
        return acc.read()
    finally:
        acc.close()


def multiline_parts(path: str, part_bytes: int, ctx=None):
    """A multi-line FASTA file in parts as the reference's reader hands them to the splitter (CFastqReader::GetPartFromMultilneFasta, fastq_reader.cpp:399-468): a title
    keeps its line end, the sequence lines lose theirs. Parts are cut in front of a '>' at a line start; a record longer than part_bytes makes its part longer.
    ctx: a BGZF file is inflated on the device (readsio.chunks)."""

    def strip(buf):
        if not buf.size:
            return buf
        start, _, end = readsio.line_table(buf) if buf[-1] == 10 else readsio.line_table(np.concatenate([buf, [10]]).astype(np.uint8))
        keep = (buf != 10) & (buf != 13)
        for s, e in zip(start[buf[start] == 62], end[buf[start] == 62]):  # titles are few: one per sequence
            keep[s:min(e, buf.size)] = True
        return buf[keep]

    held, last = [], 10  # the chunks of the part that is growing (joined once, when a cut is found: a sequence far longer than a part costs one copy), the byte before the next chunk
    for c in readsio.chunks(path, part_bytes, ctx):
        at = np.flatnonzero((c[1:] == 62) & (c[:-1] == 10)) + 1  # a '>' at a line start
        n = int(at[-1]) if at.size else (0 if held and last == 10 and c[0] == 62 else -1)
        last = int(c[-1])
        if n < 0 or (n == 0 and not held):
            held.append(c)
            continue
        buf = np.concatenate(held + [c[:n]]) if held or n < c.size else c
        if buf.size:
            yield strip(buf)
        held = [c[n:]]
    rest = np.concatenate(held) if held else np.zeros(0, dtype=np.uint8)
    if rest.size:
        yield strip(rest)


def count(argv, ctx=None, part_bytes=None, keep=False, map_multiplier=COUNT_MAP_MULTIPLIER, signature_map="fixed", output_format="kmc", input_format=None):
    """`kmc` + `kmc_tools transform sort` on the device: the reads of the input files go through a counting session (capi.CountSession) part by part, the ordered body is
    written as a KMC1 database. Returns dict(stats = the four tallies of stage 2 by name, totals = reads, super-k-mers, k-mers, bytes of bin records, n_records, n_parts,
    n_segments, n_batches, balance = k-mers of the largest bin / of the mean bin, map = the signature map that ran); keep=True: (that dict, the open session, its view) —
    the caller goes on on the device and closes the session.
    signature_map: "fixed" = count_signature_map's spread; "stats" = stage 0 first: the first part of every input file through capi.SigStats, the map from
    balanced_signature_map. With fewer than COUNT_MAP_MIN_BINS bins "stats" keeps the fixed map and the result says so. The database does not depend on the map.
    output_format: "kmc" = <out>.kmc_pre / .kmc_suf; "kff" = <out>.kff as `kmc -okff` followed by `kmc_tools transform <out>.kff reduce <out2> -okff` writes it (one
    ordered section, min_count = -ci, max_count = -cx, canonical = not -b): the session's view goes to kmc_hip_db_kff_export_device and only KFF bytes come down.
    input_format: "bam" = the inputs are BAM files, as for `kmc -fbam`: BGZF inflated on the device (kmc_hip_bgzf_inflate), the header taken off, parts of whole
    alignment records to the session with file_type 4. A bgzipped FASTA / FASTQ is recognised by its content and needs no option."""
    if signature_map not in ("fixed", "stats"):
        raise ValueError(f'count: signature_map is "fixed" or "stats", not {signature_map!r}')
    if output_format not in ("kmc", "kff"):
        raise ValueError(f'count: output_format is "kmc" or "kff", not {output_format!r}')
    bam = _input_format("count", input_format, argv)
    o = parse_count(argv)
    if bam:
        o["file_type"] = capi.SPLIT_FILE_BAM
    if part_bytes is None:
        part_bytes = int(os.environ.get("KMC_HIP_COUNT_PART_MB", "0")) << 20 or COUNT_PART_BYTES
    k = o["k"]
    own = ctx is None
    if own:
        ctx = capi.Context((0,))
    ses = None
    try:
        if signature_map == "stats" and o["n_bins"] < COUNT_MAP_MIN_BINS:
            signature_map = "fixed"
        if signature_map == "stats":
            sig_map = balanced_signature_map(count_stats_sample(ctx, o, part_bytes), o["m"], o["n_bins"], capi.allowed_signatures(o["m"], ctx.L))
            sig_map = np.where(sig_map < 0, o["n_bins"] - 1, sig_map).astype(np.int32)  # no k-mer has a signature that is not allowed; the session takes bins only
        else:
            sig_map = count_signature_map(o["m"], o["n_bins"], map_multiplier)
        ses = capi.CountSession(ctx, k, o["m"], o["n_bins"], o["both"], sig_map)
        p = ses.split_params(file_type=o["file_type"], flags=capi.SPLIT_HOMOPOLYMER if o["hc"] else 0)
        n_parts = 0
        for path in o["inputs"]:
            try:
                for i, part in enumerate(_count_parts(o, path, part_bytes, ctx)):
                    try:
                        ses.part(part, p)
                    except capi.KmcHipError as e:
                        if e.code == capi.UNCOVERED:
                            raise UsageError(f"count: {path}, part {i}: {e}")
                        raise
                    n_parts += 1
            except OSError as e:
                raise UsageError(f"cannot open file: {path} ({e.strerror})")
            except readsio.FormatError as e:
                raise UsageError(f"count: {path}: {e}")
        # the bins' own prefix length: invisible in the result; the shortest one keeps their LUTs small
        p_bins = next(q for q in range(1, 5) if (k - q) % 4 == 0)
        bp = capi.make_params(k, both_strands=1 if o["both"] else 0, cutoff_min=o["ci"], cutoff_max=o["cx"], counter_max=o["cs"], lut_prefix_len=p_bins)
        st, tot, n_records = ses.finish(bp)
        info = ses.info()
        p_out = dbio.best_lut_prefix_len(k, n_records)
        view = ses.order(p_out)
        assert view.n_recs == n_records
        _write_body(ctx, "kff" if output_format == "kff" else "kmc1", o["out"], k, view, o["ci"], o["cx"], o["both"])
        res = dict(stats=dict(zip(("n_unique", "n_below_min", "n_above_max", "n_total"), (int(x) for x in st))),
                   totals=dict(zip(("n_reads", "n_superkmers", "n_kmers", "bin_bytes"), (int(x) for x in tot))), n_records=n_records, n_parts=n_parts,
                   n_segments=info["n_segments"], n_batches=info["n_batches"], balance=info["largest_bin"] * o["n_bins"] / max(int(tot[2]), 1), map=signature_map)
        if keep:
            ses_kept, ses = ses, None
            return res, ses_kept, view
        return res
    finally:
        if ses is not None:
            ses.close()
        if own and not (keep and ses is None):
            ctx.close()


COUNT_SMALL_USAGE = """usage: python -m kmc_amd.tools count-small [options] <input_file | @file_of_inputs> <out> [<working_dir>]
  `count` for k <= 13, where `kmc` counts without signatures and bins (its small-k optimisation): -k<len> (1..13, required: kmc's default 25 belongs to `count`)
  -ci<v> (2) -cx<v> (1e9) -cs<v> (255; at least 2) -b -fa | -fq (default) | -fm -hc. -p* and -n* are accepted and ignored with the options `count` ignores. Writes
  <out>.kmc_pre / .kmc_suf byte for byte as `kmc` does for such a run (a KMC1 database, ordered as it is); with KMC_HIP_COUNT_OUT=kff <out>.kff as `kmc -okff`
  followed by `kmc_tools transform <out>.kff reduce <out2> -okff` does."""


def parse_count_small(argv) -> dict:
    """-> dict(k, ci, cx, cs, both, file_type, hc, inputs, out) of a `count-small` command line"""
    o, pos = _count_options(argv, "count-small", COUNT_SMALL_USAGE)
    if len(pos) not in (2, 3):
        raise UsageError(COUNT_SMALL_USAGE)
    k = o["k"]
    if not 1 <= k <= 13:
        raise UsageError(f"count-small: -k{k}: this verb takes k 1..13 (-k is required here); `count` is the verb for k 14..224")
    if o["ci"] < 1 or o["cs"] < 1 or o["cx"] < o["ci"]:
        raise UsageError("count-small: -ci and -cs are at least 1, -cx at least -ci")
    if o["cs"] == 1:
        raise UsageError("count-small: -cs1 stores no counter bytes at all (counter size 0): the device entries write databases with 1..4 counter bytes")
    if o["cx"] > 0xFFFFFFFF and o["cs"] > 0xFFFFFFFF:
        raise UsageError(f"count-small: -cx{o['cx']} with -cs{o['cs']} needs more than four counter bytes; a KMC database record has at most four")
    return _count_inputs(o, pos)


def smallk_lut_prefix_len(k: int, n_unique: int, counter_size: int) -> int:
    """The LUT prefix length `kmc` picks for a small-k database (ProcessSmallKOptimization_Stage2, kmc.h:906-936): the p in 1..15 with a suffix length (k - p, or 0 for
    p > k) that is a multiple of 4 and the smallest n_unique x (suffix / 4 + counter_size) + 4^p x 8, the first such p. n_unique: the NON-ZERO entries, before cutoffs."""
    best, best_mem = 0, 1 << 62
    for p in range(1, 16):
        suffix = k - p if p <= k else 0
        if suffix % 4:
            continue
        mem = n_unique * (suffix // 4 + counter_size) + (8 << (2 * p))
        if mem < best_mem:
            best, best_mem = p, mem
    return best


COUNT_SMALL_KFF_REFUSED = ()  # the k at which the reference's own KFF pipeline failed while the goldens were recorded: none


def count_small(argv, ctx=None, part_bytes=None, keep=False, output_format="kmc", input_format=None):
    """`kmc` with its small-k optimisation on the device: the reads go through capi.SmallK part by part into the table of 4^k counters, the table is tallied, the LUT
    prefix length chosen as kmc chooses it, and the table framed as the database body where it lies; only the body and the LUT come down. Returns what `count` returns
    where it has a meaning: dict(stats = n_unique, n_below_min, n_above_max, n_total; totals = n_reads, n_superkmers (0), n_kmers, bin_bytes (0); n_records, n_parts,
    file_type); keep=True: (that dict, the open capi.SmallK, its view) — the caller goes on on the device and closes the SmallK (for k <= 4 the view has no suffix bytes and
    the kmc_hip_db_* entries refuse it). output_format "kff": <out>.kff with data_size = the counter size, min_count = -ci, max_count = -cx, canonical = not -b."""
    if output_format not in ("kmc", "kff"):
        raise ValueError(f'count-small: output_format is "kmc" or "kff", not {output_format!r}')
    bam = _input_format("count-small", input_format, argv)
    o = parse_count_small(argv)
    if bam:
        o["file_type"] = capi.SPLIT_FILE_BAM
    k = o["k"]
    if output_format == "kff" and k in COUNT_SMALL_KFF_REFUSED:
        raise UsageError(f"count-small: -k{k}: the reference's own KFF pipeline fails at this k; no KFF output")
    if part_bytes is None:
        part_bytes = int(os.environ.get("KMC_HIP_COUNT_PART_MB", "0")) << 20 or COUNT_PART_BYTES
    own = ctx is None
    if own:
        ctx = capi.Context((0,))
    sk = None
    try:
        sk = capi.SmallK(ctx, k, o["both"])
        n_parts = n_reads = n_kmers = 0
        for path in o["inputs"]:
            try:
                for i, part in enumerate(_count_parts(o, path, part_bytes, ctx)):
                    try:
                        r, n = sk.part(part, file_type=o["file_type"], flags=capi.SPLIT_HOMOPOLYMER if o["hc"] else 0)
                    except capi.KmcHipError as e:
                        if e.code == capi.UNCOVERED:
                            raise UsageError(f"count-small: {path}, part {i}: {e}")
                        raise
                    n_parts, n_reads, n_kmers = n_parts + 1, n_reads + r, n_kmers + n
            except OSError as e:
                raise UsageError(f"cannot open file: {path} ({e.strerror})")
            except readsio.FormatError as e:
                raise UsageError(f"count-small: {path}: {e}")
        tally = sk.tally(o["ci"], o["cx"])
        cs = capi.counter_size(o["cx"], o["cs"], ctx.L)
        p_out = smallk_lut_prefix_len(k, tally["n_unique"], cs)
        view, st = sk.view(o["ci"], o["cx"], o["cs"], p_out)
        assert st == tally and view.n_recs == tally["n_kept"]
        if output_format == "kff":
            (d_kff, n_bytes), st = sk.view(o["ci"], o["cx"], o["cs"], framing=capi.SMALLK_KFF, data_size=cs)
            recs = np.zeros(n_bytes, dtype=np.uint8)
            if n_bytes:
                ctx.d2h(recs, d_kff)
            dbio.write_kff(o["out"] + ".kff", k, cs, o["both"], o["ci"], o["cx"], [[recs] if n_bytes else []])
            if keep:
                view, st = sk.view(o["ci"], o["cx"], o["cs"], p_out)
        else:
            _write_smallk_body(ctx, o["out"], k, view, o["ci"], o["cx"], o["both"])
        res = dict(stats=dict(n_unique=tally["n_unique"], n_below_min=tally["n_cutoff_min"], n_above_max=tally["n_cutoff_max"], n_total=n_kmers),
                   totals=dict(n_reads=n_reads, n_superkmers=0, n_kmers=n_kmers, bin_bytes=0), n_records=tally["n_kept"], n_parts=n_parts, file_type=o["file_type"])
        if keep:
            sk_kept, sk = sk, None
            return res, sk_kept, view
        return res
    finally:
        if sk is not None:
            sk.close()
        if own and not (keep and sk is None):
            ctx.close()


SMALLK_BODY_PART_BYTES = 64 << 20


def _write_smallk_body(ctx, path: str, k: int, body: capi.DbView, ci: int, cx: int, both_strands: bool):
    """_write_body's "kmc1" for a small-k view: the prefix may be the whole k-mer (k <= 4: no suffix bytes), and a large body comes down in parts"""
    n, p, cs = int(body.n_recs), int(body.lut_prefix_len), int(body.counter_size)
    if p < k and n * ((k - p) // 4 + cs) <= SMALLK_BODY_PART_BYTES:
        return _write_body(ctx, "kmc1", path, k, body, ci, cx, both_strands)
    recs, lut = np.zeros(n * ((k - p) // 4 + cs), dtype=np.uint8), np.zeros(1 << (2 * p), dtype=np.uint64)
    for at in range(0, recs.size, SMALLK_BODY_PART_BYTES):
        ctx.d2h(recs[at:at + SMALLK_BODY_PART_BYTES], body.d_recs + at)
    ctx.d2h(lut, body.d_lut)
    dbio.write_kmc1(path, k, cs, p, ci, cx, both_strands, lut, recs)


def count_report(res: dict) -> str:
    """the lines of `kmc`'s summary (kmc_CLI/kmc.cpp:410-419) + the bins' balance, where the run had bins (`count-small` has none)"""
    s, t = res["stats"], res["totals"]
    rows = [("No. of k-mers below min. threshold", s["n_below_min"]), ("No. of k-mers above max. threshold", s["n_above_max"]), ("No. of unique k-mers", s["n_unique"]),
            ("No. of unique counted k-mers", s["n_unique"] - s["n_below_min"] - s["n_above_max"]), ("Total no. of k-mers", s["n_total"]),
            ("Total no. of sequences" if res.get("file_type") == 2 else "Total no. of reads", t["n_reads"]), ("Total no. of super-k-mers", t["n_superkmers"])]
    text = "\n".join("   %-35s: %12d" % r for r in rows)
    if "balance" not in res:
        return text
    which = {"fixed": "the fixed signature map", "stats": "the map from stage-0 statistics"}[res.get("map", "fixed")]
    return text + "\n   %-35s: %12.2f  (%s; %d parts, %d segments gathered, %d stage-2 batches)" % (
        "Largest bin / mean bin (k-mers)", res["balance"], which, res["n_parts"], res["n_segments"], res["n_batches"])


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "count":
        print(count_report(count(argv[1:], signature_map="stats" if os.environ.get("KMC_HIP_COUNT_MAP") == "stats" else "fixed",
                                 output_format="kff" if os.environ.get("KMC_HIP_COUNT_OUT") == "kff" else "kmc",
                                 input_format="bam" if os.environ.get("KMC_HIP_COUNT_IN") == "bam" else None)))
        return 0
    if argv and argv[0] == "count-small":
        print(count_report(count_small(argv[1:], output_format="kff" if os.environ.get("KMC_HIP_COUNT_OUT") == "kff" else "kmc",
                                       input_format="bam" if os.environ.get("KMC_HIP_COUNT_IN") == "bam" else None)))
        return 0
    if argv and argv[0] == "export":
        out = parse_export(argv[1:])[1]["path"]
        print(f"export -> {out}.kff: " + ", ".join(f"{a} {b}" for a, b in export(argv[1:]).items()))
        return 0
    if argv and argv[0] == "filter":
        print(", ".join(f"{a} {b}" for a, b in filter_reads(argv[1:]).items()))
        return 0
    if argv and argv[0] == "transform":
        outs = [o for o in parse_transform(argv[1:])[1]]
        sts = transform(argv[1:])
        if len(sts) != len(outs):  # an ordered input: the sorts were left out
            outs = [o for o in outs if o["op"] != "sort"]
        for (o, st) in zip(outs, sts):
            print(f"{o['op']} -> {o['path']}: " + ", ".join(f"{a} {b}" for a, b in st.items()))
        return 0
    if argv and argv[0] == "complex":
        st = complex(argv[1:])
        print(f"complex -> {parse_complex(open(argv[1]).read())['path']}: " + ", ".join(f"{a} {b}" for a, b in st.items()))
        return 0
    if argv and argv[0] == "compare":
        res = compare(argv[1:])
        sys.stdout.write(compare_report(res))
        return 0 if res["kind"] == "equal" else 1  # kmc_tools.cpp:518-527: exit(0), exit(1)
    if argv and argv[0] == "check":
        sys.stdout.write(check(argv[1:]))
        return 0
    if argv and argv[0] == "info":
        out, err = info(argv[1:])
        sys.stdout.write(out)
        sys.stderr.write(err)
        return 0
    if not argv or argv[0] != "simple":
        raise UsageError("usage: python -m kmc_amd.tools simple <db1> [-ci -cx] <db2> [-ci -cx] <operation> <out> [-ci -cx -cs -oc<mode>] ...\n" + FILTER_USAGE + "\n" + TRANSFORM_USAGE + "\n"
                         + COMPLEX_USAGE + "\n" + COMPARE_USAGE + "\n" + CHECK_USAGE + "\n" + INFO_USAGE + "\n" + COUNT_USAGE + "\n" + COUNT_SMALL_USAGE + "\n" + EXPORT_USAGE)
    for (o, st) in zip(parse_simple(argv[1:])[1], simple(argv[1:])):
        print(f"{o['op']} -> {o['path']}: " + ", ".join(f"{a} {b}" for a, b in st.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
