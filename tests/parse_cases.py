"""Inputs for the tests of result text parsed on the device (k_parse.hip, mtsv_fold_add_text, mtsv-collapse --on-gpu): shared by
test_parse_text_cpu.py and test_parse_text.py.  Texts only; what they must give comes from parse_ref.py or the host tool."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mtsv_tools_amd", "bin", "mtsv-collapse")
GOLDEN = os.path.join(ROOT, "tests", "golden")
TILE = 64
# every digit count, both ends of the range, and values with bit 31 set
VALUES = [0, 9, 10, 99, 100, 12345, 999999, 1000000, 99999999, 123456789, 999999999, 1000000000, 2147483648, 4294967295]


def edge_lines(seed=11, n_lines=420):
    """[(read, hits)]: long tokens of every length from 7 to 43 bytes, keys ascending by (tax, gi, offset) inside a line (so
    the lines are legal at every grain, with runs of equal keys at the two coarser ones), reads with gaps, an empty line now
    and then.  About 40 KiB: several tiles of 4096 bytes, hundreds of 64."""
    rng = random.Random(seed)
    lines, read = [], 0
    for j in range(n_lines):
        read += rng.randrange(1, 4)
        if j % 37 == 5:
            lines.append((read, ""))
            continue
        keys = set()
        for _ in range(rng.randrange(1, 9)):
            tax = rng.choice(VALUES[:6]) if rng.random() < 0.7 else rng.choice(VALUES)
            keys.add((tax, rng.choice(VALUES[:4] + VALUES[-3:]), rng.choice(VALUES)))
        lines.append((read, ",".join(f"{t}-{g}-{o}={rng.choice(VALUES)}" for t, g, o in sorted(keys))))
    return lines


def edge_coverage(lines, tile):
    """the offsets within a tile at which a token starts, at which one ends (its last byte), at which a ',' stands and at
    which a non-empty line starts"""
    starts, ends, commas, slots = set(), set(), set(), set()
    at = 0
    for _, h in lines:
        if h:
            slots.add(at % tile)
        p = at
        for tok in h.split(",") if h else []:
            starts.add(p % tile)
            ends.add((p + len(tok) - 1) % tile)
            p += len(tok) + 1
            commas.add((p - 1) % tile)
        at += len(h)
    return starts, ends, commas, slots


REFERENCE = {  # the reference's own vectors (src/collapse.rs:788-817), as tests/test_collapse.py holds them
    "taxid": (["r1:1=5,2=9\nr2:3=4", "r1:1=2,2=10\nr2:3=1"], "r1:1=2,2=9\nr2:3=1\n"),
    "taxid-gi": (["r1:1-5-3=7,1-5-2=4\nr2:2-9-1=3", "r1:1-5-4=5,2-8-1=6\nr2:2-9-1=2"], "r1:1-5-2=4,2-8-1=6\nr2:2-9-1=2\n"),
}
REPORT_INPUT = ["a:1=0,2=3\nb:1=2\nc:1=1,2=1"]


def golden_cut(name):
    """a golden results file cut into three overlapping files: lines [0, 60), [40, 110) and [90, end) with every edit of the
    second file raised by one and its lines reversed"""
    lines = open(os.path.join(GOLDEN, name)).read().splitlines()
    assert len(lines) == 140
    bump = lambda l: l.rsplit(":", 1)[0] + ":" + ",".join(f"{t.split('=')[0]}={int(t.split('=')[1]) + 1}" for t in l.rsplit(":", 1)[1].split(","))  # noqa: E731
    return ["\n".join(lines[:60]) + "\n", "\r\n".join(bump(l) for l in reversed(lines[40:110])) + "\r\n", "\n".join(lines[90:])]


COLON_IDS = ["x:y:1-2-3=4,1-2-9=1\nx:1-1-1=1\n\n \t\nx:y:z:7-7-7=7\n", "x:y:1-2-3=2\nx:y:z:7-7-7=9,8-1-1=0\n:x:5-5-5=5\n"]
LAYERS = ["q:3-1-1=5\np:1-1-1=4\nq:1-1-1=9,3-1-1=2\nq:3-1-0=7\nz:\np:1-1-1=6\n", "q:2-2-2=2\n"]
KEY_ORDER = ["a:1-1-1=1,2-1-1=1\nb:5-1-1=1,4-1-1=1\n", "a:3-1-1=3\n"]       # the second line of the first file descends
NO_OFFSET = ["a:1-5=7,1-5=4\nb:2-9=3\n", "a:1-5=5,2-8=6\n"]               # T-G=E: the device writes no such form
MALFORMED = ["a:1-1-1=1\nb:1-1-x=2\n"]


def run_tool(tmp_path, texts, *extra, env=None, tag="out"):
    """(CompletedProcess, output bytes or None, report bytes or None) of mtsv-collapse on the texts written as files"""
    paths = []
    for i, t in enumerate(texts):
        p = tmp_path / f"{tag}_in{i}.txt"
        p.write_bytes(t.encode("latin-1"))
        paths.append(str(p))
    out, rep = tmp_path / f"{tag}.txt", tmp_path / f"{tag}.tsv"
    r = subprocess.run([BIN, "-o", str(out), "--report", str(rep), *extra, *paths], capture_output=True, text=True,
                       env=dict(os.environ, **(env or {})))
    return r, (out.read_bytes() if out.exists() else None), (rep.read_bytes() if rep.exists() else None)
