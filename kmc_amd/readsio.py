"""Reads files <-> numpy for `python -m kmc_amd.tools filter`: 4-line FASTQ or 2-line FASTA text cut into records the way CFastqFilter::NextSeqFastq and NextSeqFasta
do (kmc_tools/fastq_filter.cpp:179-339), as arrays of offsets into the text — nothing is copied per read.

Those parsers stop at the first record they cannot read and the rest of the part is silently lost. Here such text raises FormatError instead: a lead character other
than '@' / '+' / '>', a quality line that is not as long as its sequence, an empty line, a control character or a byte above 127 other than the line ends, a last record without
its line end. Line ends are '\\n' or '\\r\\n'."""
from __future__ import annotations

import gzip
import os
from dataclasses import dataclass

import numpy as np


class FormatError(ValueError):
    pass


@dataclass
class Records:
    """Spans [start, end) into `text`, one entry per record; an end is the end of the line's content, in front of its '\\r\\n' or '\\n'. plus and qual are None for FASTA."""
    text: np.ndarray  # uint8
    header: tuple
    seq: tuple
    plus: tuple
    qual: tuple
    rec_end: np.ndarray  # the start of the next record

    def __len__(self):
        return self.rec_end.size


def line_table(text: np.ndarray):
    """-> (start, content end, end behind the line end) of every complete line"""
    nl = np.flatnonzero(text == 10)
    start = np.concatenate([[0], nl[:-1] + 1]) if nl.size else nl
    cr = (nl > start) & (text[np.maximum(nl, 1) - 1] == 13)
    return start, nl - cr, nl + 1


def whole_records(text: np.ndarray, fastq: bool) -> int:
    """bytes of `text` that are whole records (lines in fours or twos): what a part of a file may hold; the rest belongs to the next part"""
    _, _, end = line_table(text)
    per = 4 if fastq else 2
    n = end.size // per * per
    return int(end[n - 1]) if n else 0


def parse(text, fastq: bool) -> Records:
    """text: bytes or uint8 array holding whole records."""
    text = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.asarray(text, dtype=np.uint8)
    kind = "FASTQ" if fastq else "FASTA"
    if text.size and text[-1] != 10:
        raise FormatError(f"{kind}: the last record has no line end")
    start, cend, end = line_table(text)
    per = 4 if fastq else 2
    if start.size % per:
        raise FormatError(f"{kind}: {start.size} lines, not a multiple of {per}")
    if np.count_nonzero((text < 32) | (text >= 128)) != start.size + np.count_nonzero(cend + 1 != end):  # `char c; c < 32` ends a line there
        raise FormatError(f"{kind}: a control character or a byte above 127 that is not a line end")
    lead = text[start] if start.size else start
    if np.any(cend == start):  # an empty line has no lead character (and the reference takes the next line for it)
        raise FormatError(f"{kind}: empty line {int(np.flatnonzero(cend == start)[0]) + 1}")
    if np.any(lead[0::per] != ord("@" if fastq else ">")):
        raise FormatError(f"{kind}: record {int(np.flatnonzero(lead[0::per] != ord('@' if fastq else '>'))[0]) + 1} does not start with '{'@' if fastq else '>'}'")
    span = lambda j: (start[j::per], cend[j::per])  # noqa: E731
    if not fastq:
        return Records(text, span(0), span(1), None, None, end[1::per])
    if np.any(lead[2::per] != ord("+")):
        raise FormatError(f"FASTQ: record {int(np.flatnonzero(lead[2::per] != ord('+'))[0]) + 1} has no '+' line")
    r = Records(text, span(0), span(1), span(2), span(3), end[3::per])
    bad = (r.qual[1] - r.qual[0]) != (r.seq[1] - r.seq[0])
    if np.any(bad):
        raise FormatError(f"FASTQ: record {int(np.flatnonzero(bad)[0]) + 1}: the quality line is not as long as the sequence")
    return r


def gather(src: np.ndarray, starts: np.ndarray, ends: np.ndarray) -> np.ndarray:
    """the bytes src[starts[i]:ends[i]] of every i, one after the other"""
    starts, lens = np.asarray(starts, dtype=np.int64).ravel(), (np.asarray(ends, dtype=np.int64) - np.asarray(starts, dtype=np.int64)).ravel()
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, dtype=np.uint8)
    at = np.cumsum(lens) - lens
    return src[np.arange(total, dtype=np.int64) - np.repeat(at - starts, lens)]


def sequence_buffer(rec: Records):
    """-> (uint8: every record's sequence line followed by one '\\n', uint64 offsets[n + 1]): the input of kmc_hip_db_query_reads_device"""
    lens = (rec.seq[1] - rec.seq[0]).astype(np.int64)
    off = np.zeros(lens.size + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens + 1)
    buf = gather(rec.text, rec.seq[0], rec.seq[1] + 1)  # the byte behind the content is '\r' or '\n'
    if buf.size:
        buf[off[1:].astype(np.int64) - 1] = 10
    return buf, off


def is_bgzf(path: str) -> bool:
    """the file's first gzip member has the BC subfield of length 2 in its extra field: BGZF (BAM, bgzip), not plain gzip"""
    with open(path, "rb") as f:
        h = f.read(12)
        if len(h) < 12 or h[:3] != b"\x1f\x8b\x08" or not h[3] & 4:
            return False
        extra = f.read(h[10] | h[11] << 8)
    x = 0
    while x + 4 <= len(extra):
        slen = extra[x + 2] | extra[x + 3] << 8
        if extra[x:x + 2] == b"BC" and slen == 2 and x + 6 <= len(extra):
            return True
        x += 4 + slen
    return False


def on_device(path: str, ctx) -> bool:
    """do this file's bytes come from the device inflate? a context is given, $KMC_HIP_BGZF is not 0 and the file is BGZF"""
    return ctx is not None and os.environ.get("KMC_HIP_BGZF", "1") != "0" and is_bgzf(path)


def bgzf_chunks(path: str, ctx, part_bytes: int, piece_bytes: int = None):
    """A BGZF file's inflated bytes as uint8 arrays of about part_bytes, inflated on the device (capi.bgzf_inflate): the file is read in compressed pieces
    ($KMC_HIP_BGZF_PIECE bytes, by default a quarter of part_bytes), each piece's member table comes from capi.bgzf_scan, the incomplete last member is carried in
    front of the next piece. A member that is not BGZF, a member the device refuses and a file that ends inside a member raise FormatError with the file offset."""
    from . import capi

    if piece_bytes is None:
        piece_bytes = int(os.environ.get("KMC_HIP_BGZF_PIECE", "0")) or max(part_bytes // 4, 1 << 16)
    carry, base = np.zeros(0, dtype=np.uint8), 0  # base: the file offset of carry[0]
    with open(path, "rb") as f:
        while True:
            piece = f.read(piece_bytes)
            buf = np.concatenate([carry, np.frombuffer(piece, dtype=np.uint8)]) if carry.size else np.frombuffer(piece, dtype=np.uint8)
            pos = 0
            while pos < buf.size:
                try:
                    members, used, out_bytes = capi.bgzf_scan(buf[pos:], part_bytes, L=ctx.L)
                    if not members.size:  # a member of more than part_bytes (it holds at most 64 KiB) goes alone
                        members, used, out_bytes = capi.bgzf_scan(buf[pos:], 1 << 16, cap=1, L=ctx.L)
                except capi.KmcHipError as e:
                    msg, _, at = str(e).rpartition(" at byte ")
                    raise FormatError(f"BGZF: {msg.split(': ', 2)[-1]} at byte {base + pos + int(at)} of the file")
                if not members.size:
                    break
                try:
                    out = capi.bgzf_inflate(ctx, buf[pos:pos + used], members)
                    if out.size:
                        yield out
                except capi.BgzfError as e:
                    raise FormatError(f"BGZF: the member whose compressed data starts at byte {base + pos + int(members['src_off'][e.first_bad])} of the file is corrupt: "
                                      + str(e).rpartition("): ")[2])
                pos += used
            carry, base = buf[pos:], base + pos
            if not piece:
                break
    if carry.size:
        raise FormatError(f"BGZF: the file ends inside the member at byte {base}")


def chunks(path: str, part_bytes: int, ctx=None, gz: bool = None):
    """the file's (inflated) bytes as uint8 arrays of about part_bytes: from the device where on_device() says so, else through gzip (gz, by default a name that ends
    in .gz) or as they are"""
    if on_device(path, ctx):
        yield from bgzf_chunks(path, ctx, part_bytes)
        return
    with (gzip.open(path, "rb") if (path.endswith(".gz") if gz is None else gz) else open(path, "rb")) as f:
        while True:
            chunk = f.read(part_bytes)
            if not chunk:
                break
            yield np.frombuffer(chunk, dtype=np.uint8)


def parts(path: str, fastq: bool, part_bytes: int, ctx=None):
    """yields the file's text in parts of whole records of about part_bytes. ctx (a capi.Context, or anything with its L and h): a BGZF file is inflated on the device"""
    rest = np.zeros(0, dtype=np.uint8)
    for chunk in chunks(path, part_bytes, ctx):
        buf = np.concatenate([rest, chunk])
        n = whole_records(buf, fastq)
        if n:
            yield buf[:n]
        rest = buf[n:]
    if rest.size:
        yield rest  # no whole record: parse() says what is wrong with it


def bam_parts(path: str, part_bytes: int, ctx):
    """A BAM file as the reference's BAM reader hands it to the splitter (CFastqReader::GetPartFromBam, kmc_core/fastq_reader.cpp:191-362): the inflated stream without
    its header (magic, l_text, text, n_ref, references — over however many members), in parts of whole alignment records (capi.bam_whole_records); what is left of
    a record goes in front of the next chunk. No magic, a damaged block_size and a stream that ends inside the header or a record raise FormatError."""
    from . import capi

    def header_bytes(b):
        """the header's length, or None while b does not hold all of it"""
        if b.size < 12:
            return None
        at = 8 + int(b[4:8].view("<i4")[0])
        if at < 8:
            raise FormatError("BAM: negative l_text")
        if b.size < at + 4:
            return None
        n_ref = int(b[at:at + 4].view("<i4")[0])
        at += 4
        for _ in range(max(n_ref, 0)):
            if b.size < at + 4:
                return None
            l_name = int(b[at:at + 4].view("<i4")[0])
            if l_name < 0:
                raise FormatError("BAM: negative l_name")
            at += 4 + l_name + 4
        return at if b.size >= at else None

    buf, in_header = np.zeros(0, dtype=np.uint8), True
    for chunk in chunks(path, part_bytes, ctx, gz=True):
        buf = np.concatenate([buf, chunk]) if buf.size else chunk
        if in_header:
            if buf.size >= 4 and buf[:4].tobytes() != b"BAM\1":
                raise FormatError("BAM: the inflated stream does not start with the magic BAM\\1")
            n = header_bytes(np.ascontiguousarray(buf))
            if n is None:
                continue
            buf, in_header = buf[n:], False
        try:
            n, _ = capi.bam_whole_records(buf, L=ctx.L)
        except capi.KmcHipError as e:
            raise FormatError("BAM: " + str(e).split(": ", 2)[-1])
        if n:
            yield buf[:n]
        buf = buf[n:]
    if in_header:
        raise FormatError("BAM: the stream ends inside the header" if buf.size >= 4 else "BAM: the inflated stream does not start with the magic BAM\\1")
    if buf.size:
        raise FormatError(f"BAM: the stream ends inside a record ({buf.size} bytes left over)")
