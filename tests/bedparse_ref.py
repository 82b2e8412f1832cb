"""Plain Python restatement of the BED line / field rule over raw bytes (trackIO.bedRead is the specification; the
device parse of tehmm_bedparse.hip.h is held to this restatement), the corpus both suites run it on, and the number
texts and their certification domain.  Needs no library."""
import random
import re


def lineSpans(data):
    """[(start, end)] of every line's bytes without its terminator: "\\n", "\\r\\n" or a lone "\\r" ends a line, a
    last line without a terminator counts"""
    out, i, n, start = [], 0, len(data), 0
    while i < n:
        b = data[i:i + 1]
        if b == b"\n":
            out.append((start, i))
            start = i = i + 1
        elif b == b"\r":
            out.append((start, i))
            i += 2 if data[i + 1:i + 2] == b"\n" else 1
            start = i
        else:
            i += 1
    if start < n:
        out.append((start, n))
    return out


def records(data):
    """kept records: [(start, end, [(field start, field length)])]: no '#' as the line's first byte, three fields"""
    out = []
    for a, b in lineSpans(data):
        if data[a:a + 1] == b"#":
            continue
        fields, f0 = [], a
        for q in range(a, b + 1):
            if q == b or data[q:q + 1] == b"\t":
                fields.append((f0, q - f0))
                f0 = q + 1
        if len(fields) > 2:
            out.append((a, b, fields))
    return out


def fieldTexts(data):
    """what bedRead returns for a file of these bytes (ASCII)"""
    return [[data[a:a + n].decode("ascii") for a, n in fields] for _, _, fields in records(data)]


def numLines(data):
    return len(lineSpans(data))


def tables(data, ncols=6):
    """(line starts, line lengths, field counts, [record][ncols] offsets from the line start, lengths, -1: no column)"""
    recs = records(data)
    off = [[f[k][0] - a if k < len(f) else 0 for k in range(ncols)] for a, _, f in recs]
    length = [[f[k][1] if k < len(f) else -1 for k in range(ncols)] for _, _, f in recs]
    return [a for a, _, _ in recs], [b - a for a, b, _ in recs], [len(f) for _, _, f in recs], off, length


# ---- corpus -------------------------------------------------------------------------------------------------------------
ALPHABET = [b"\t", b"\n", b"\r", b"#", b"a", b"1", b" ", b"."]


def corpus():
    """[(name, bytes)]"""
    twelve = b"\t".join([b"chr1", b"10", b"20"] + [b"f%d" % k for k in range(9)])
    return [
        ("terminators_mixed", b"c\t1\t2\nc\t3\t4\r\nc\t5\t6\rc\t7\t8\n"),
        ("cr_cr_lf", b"c\t1\t2\r\r\nc\t3\t4\r\r\n"),
        ("lf_cr", b"c\t1\t2\n\rc\t3\t4\n\r"),
        ("no_last_terminator", b"c\t1\t2\nc\t3\t4"),
        ("last_is_cr", b"c\t1\t2\nc\t3\t4\r"),
        ("empty", b""),
        ("only_terminators", b"\n\r\n\r\r\n\n"),
        ("one_lf", b"\n"),
        ("comments", b"#head\tx\ty\nc\t1\t2\n#c\t3\t4\r\nc\t5\t6\r#x\ty\tz\rc\t7\t8"),
        ("hash_in_field", b"c\t1\t2\t#name\nc#\t3\t4\n\t#\t5\t6\n"),
        ("field_counts", b"one\none\ttwo\nc\t1\t2\n" + twelve + b"\n"),
        ("empty_fields", b"\t\t\nc\t\t2\t\tx\n\t1\t2\n"),
        ("trailing_tab", b"c\t1\t2\t\nc\t1\t\n"),
        ("blanks", b" c \t 1\t2 \t a b \n  \t \t \n"),
        ("two_fields_cr", b"a\tb\rc\t1\t2\r"),
        ("comment_only", b"#\n#\r\n#"),
    ]


def randomFiles(count=200, seed=20240607):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        n = rng.choice([0, 1, 2, 3, 15, 16, 17, 40, 100, 300])
        weights = rng.choice([[3, 2, 2, 1, 4, 4, 1, 1], [1, 1, 1, 1, 1, 1, 1, 1], [6, 1, 1, 1, 2, 2, 1, 1]])
        out.append(b"".join(rng.choices(ALPHABET, weights=weights, k=n)))
    return out


# ---- numbers ------------------------------------------------------------------------------------------------------------
INT_CERTIFIED = ["0", "7", "-0", "+0", "007", "-12", "+34", "123456789", "999999999999999999", "-999999999999999999",
                 "000000000000000001"]
INT_HOST = ["", " 1", "1 ", "1_0", "+", "-", "1234567890123456789", "1.0", "12x", "--", "0x10", "1e3"]

FLOAT_CRAFTED = ["1e22", "1e23", "9007199254740993", "123456789012345", "1234567890123456", "0.123456789012345",
                 "0.1234567890123456", ".5", "5.", ".", "e5", "-0.0", "0e999", "inf", "nan", "0x10", "1_0.5", "1.5e-21",
                 "1.5e-22", "1.5e-23", "15e-23", "1e-22", "3.0", "0.1", "-2.5E+3", "+7.25", "1e+22", "1.e5", "00012.500", "", "-",
                 "1e", "1e+", "1.2.3", " 1.0", "1.0 ", "-.5e-1", "000000000000000000000.000000000000000000001e-1",
                 "123456789012345e22", "123456789012345e23", "0.0000000000000000000001", "1e0005", "12345678901234500"]

_FLOAT_RE = re.compile(r"[+-]?(\d*)(?:\.(\d*))?(?:[eE]([+-]?\d+))?", re.ASCII)


def floatInDomain(text):
    """The certified domain, from the rule: plain syntax, at most 15 significant digits (the first non-zero digit to
    the mantissa's last digit), |exponent - fraction digits| <= 22; a mantissa of zeros is in it"""
    m = _FLOAT_RE.fullmatch(text)
    if not m or text.count(".") > 1:
        return False
    ip, fp = m.group(1) or "", m.group(2) or ""
    digits = ip + fp
    if not digits:
        return False
    sig = digits.lstrip("0")
    if not sig:
        return True
    return len(sig) <= 15 and abs(int(m.group(3) or 0) - len(fp)) <= 22


def intInDomain(text):
    return re.fullmatch(r"[+-]?[0-9]{1,18}", text, re.ASCII) is not None


def randomFloatTexts(count=100000, seed=77):
    """decimal texts with 1 to 20 significant digits, optional point, optional exponent |e10| <= 30, leading and
    trailing zeros"""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        nsig = rng.randint(1, 20)
        digits = str(rng.randint(1, 9)) + "".join(rng.choice("0123456789") for _ in range(nsig - 1))
        digits = "0" * rng.choice([0, 0, 1, 3]) + digits + "0" * rng.choice([0, 0, 0, 1, 2])
        if rng.random() < 0.1:
            digits = "0" * rng.randint(1, 5)
        text = digits
        if rng.random() < 0.7:
            p = rng.randint(0, len(digits))
            text = digits[:p] + "." + digits[p:]
        if rng.random() < 0.5:
            text += rng.choice("eE") + rng.choice(["", "+", "-"]) + str(rng.randint(0, 30))
        out.append(rng.choice(["", "", "-", "+"]) + text)
    return out
