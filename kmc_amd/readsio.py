"""Reads files <-> numpy for `python -m kmc_amd.tools filter`: 4-line FASTQ or 2-line FASTA text cut into records the way CFastqFilter::NextSeqFastq and NextSeqFasta
do (kmc_tools/fastq_filter.cpp:179-339), as arrays of offsets into the text — nothing is copied per read.

Those parsers stop at the first record they cannot read and the rest of the part is silently lost. Here such text raises FormatError instead: a lead character other
than '@' / '+' / '>', a quality line that is not as long as its sequence, an empty line, a control character or a byte above 127 other than the line ends, a last record without
its line end. Line ends are '\\n' or '\\r\\n'."""
from __future__ import annotations

import gzip
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


def parts(path: str, fastq: bool, part_bytes: int):
    """yields the file's text in parts of whole records of about part_bytes"""
    rest = np.zeros(0, dtype=np.uint8)
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        while True:
            chunk = f.read(part_bytes)
            if not chunk:
                break
            buf = np.concatenate([rest, np.frombuffer(chunk, dtype=np.uint8)])
            n = whole_records(buf, fastq)
            if n:
                yield buf[:n]
            rest = buf[n:]
    if rest.size:
        yield rest  # no whole record: parse() says what is wrong with it
