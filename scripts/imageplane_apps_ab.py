"""Compares what scripts/imageplane_apps_ab.sh wrote: A1, A2 (the other build's programs, twice) and B (this tree's).  stdout must be identical apart from
the numbers of the timing line, stderr and FITS headers byte for byte, and every number of B within the difference of A1 and A2 from each other (0: bit
for bit).
  scripts/imageplane_apps_ab.py [output directory, default build/imageplane_apps_ab]"""
import glob
import os
import re
import sys

import numpy as np

O = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "imageplane_apps_ab")
NUM = re.compile(r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?")


def masked_stdout(path):
    return [NUM.sub("#", line) if line.startswith("timing:") else line for line in open(path).read().splitlines()]


def fits_hdus(path):
    """[(header bytes, data as float64 array)]"""
    raw = open(path, "rb").read()
    out, pos = [], 0
    while pos < len(raw):
        start, cards = pos, {}
        while True:
            block = raw[pos:pos + 2880]
            pos += 2880
            done = False
            for i in range(0, 2880, 80):
                card = block[i:i + 80].decode("ascii")
                if card.startswith("END"):
                    done = True
                    break
                if card[8:10] == "= ":
                    cards[card[:8].strip()] = card[10:].split("/")[0].strip()
            if done:
                break
        header = raw[start:pos]
        naxis = int(cards.get("NAXIS", 0))
        count = int(np.prod([int(cards[f"NAXIS{i + 1}"]) for i in range(naxis)])) if naxis else 0
        bitpix = int(cards.get("BITPIX", 8))
        nbytes = count * abs(bitpix) // 8
        assert bitpix == -64 or count == 0, (path, bitpix)
        data = np.frombuffer(raw[pos:pos + nbytes], dtype=">f8").astype(np.float64)
        pos += (nbytes + 2879) // 2880 * 2880
        out.append((header, data))
    return out


def rel(a, b):
    """largest |a - b| / max(|a|, |b|); NaN against NaN and equal values count 0, NaN against a number counts inf"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if a.shape != b.shape:
        return float("inf")
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    if same.all():
        return 0.0
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))
    d[same] = 0
    d[np.isnan(d)] = np.inf
    return float(d.max())


def text_numbers(path):
    return np.array([float(t) for t in open(path).read().split() if NUM.fullmatch(t) or t in ("nan", "-nan")])


ok = True
for b_path in sorted(glob.glob(os.path.join(O, "B", "*"))):
    name = os.path.basename(b_path)
    a1, a2 = os.path.join(O, "A1", name), os.path.join(O, "A2", name)
    if name.endswith(".stderr"):
        good = open(a1).read() == open(b_path).read()
        print(f"{name:34s} stderr identical: {good}")
    elif name.endswith(".stdout"):
        good = masked_stdout(a1) == masked_stdout(b_path) and masked_stdout(a1) == masked_stdout(a2)
        print(f"{name:34s} stdout identical apart from the numbers of the timing line: {good}")
    elif name.endswith(".fits"):
        h1, h2, hb = fits_hdus(a1), fits_hdus(a2), fits_hdus(b_path)
        headers = [x[0] for x in h1] == [x[0] for x in hb] and len(h1) == len(hb)
        self_d = max(rel(x[1], y[1]) for x, y in zip(h1, h2))
        new_d = max(rel(x[1], y[1]) for x, y in zip(h1, hb))
        bytes_same = open(a1, "rb").read() == open(b_path, "rb").read()
        good = headers and new_d <= self_d
        print(f"{name:34s} {len(hb)} HDUs, headers identical: {headers}; data: parent vs parent {self_d:.3g}, new vs parent {new_d:.3g}; file bytes identical: {bytes_same}")
    else:
        self_d, new_d = rel(text_numbers(a1), text_numbers(a2)), rel(text_numbers(a1), text_numbers(b_path))
        bytes_same = open(a1, "rb").read() == open(b_path, "rb").read()
        good = new_d <= self_d
        print(f"{name:34s} text: parent vs parent {self_d:.3g}, new vs parent {new_d:.3g}; file bytes identical: {bytes_same}")
    ok = ok and good
print("A/B:", "PASS" if ok else "FAIL")
sys.exit(0 if ok else 1)
