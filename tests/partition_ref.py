"""Python restatement of read partitioning (mtsv-partition, mtsv-binner --matched / --unmatched), for the tests.

A record is (id, desc, seq, qual) in bytes: `id` the first token of the header line (split at the first space or tab),
`desc` the rest of the header after that one separator with trailing whitespace removed (b"" when there is none), `seq`
the bases as they stand in the file with wrapped lines joined, `qual` the quality string (None for FASTA).

Written out again a record is
    FASTA   >ID[ DESC]\\nSEQ\\n
    FASTQ   @ID[ DESC]\\nSEQ\\n+\\nQUAL\\n
with DESC and its space left out when DESC is empty.  A record goes to the matched side when its ID is in the set of
IDs of the results files (the standalone tool: records that share an ID share a fate) or when its flag is set (the
binner's fused mode: every read by itself), else to the unmatched side; both sides keep the input order."""

WHITESPACE = b" \t\r\n\v\f"


def split_header(header):
    """(id, desc) of a header line without its marker and line end"""
    cut = len(header)
    for k, c in enumerate(header):
        if c in b" \t":
            cut = k
            break
    return header[:cut], header[cut + 1:].rstrip(WHITESPACE)


def record_bytes(rec, fastq):
    rid, desc, seq, qual = rec
    head = (b"@" if fastq else b">") + rid + (b" " + desc if desc else b"") + b"\n"
    if fastq:
        assert qual is not None and len(qual) == len(seq)
        return head + seq + b"\n+\n" + qual + b"\n"
    return head + seq + b"\n"


def partition_by_flags(records, flags, fastq):
    """(matched bytes, unmatched bytes): record k goes to the matched side when flags[k] is true"""
    assert len(records) == len(flags)
    out = ([], [])
    for rec, f in zip(records, flags):
        out[0 if f else 1].append(record_bytes(rec, fastq))
    return b"".join(out[0]), b"".join(out[1])


def partition_by_ids(records, ids, fastq):
    """(matched bytes, unmatched bytes): a record goes to the matched side when its ID is in `ids`"""
    return partition_by_flags(records, [rec[0] in ids for rec in records], fastq)


class InvalidHeader(ValueError):
    pass


def ids_from_results(texts):
    """the IDs of results files given as bytes: lines that are empty after trimming are skipped, the ID is everything
    before the last ':' of a line; a line without ':' or with an empty ID raises InvalidHeader(line)"""
    ids = set()
    for text in texts:
        for line in text.split(b"\n"):
            if line.endswith(b"\r"):
                line = line[:-1]
            if not line.strip(WHITESPACE):
                continue
            rid, sep, _ = line.rpartition(b":")
            if not sep or not rid:
                raise InvalidHeader(line)
            ids.add(rid)
    return ids
