"""Shared by tests/test_jpeg_size_cpu.py, tests/test_gpu_jpeg_size.py and tests/golden/make_jpeg_sizes.py: seeded image recipes for the JPEG byte
counter and a small baseline-JPEG stream parser (what the encoder under comparison really wrote: header length, stuffed bytes, bits, ZRL symbols)."""
import json
import os

import numpy as np

RECIPES = ("noise", "smooth", "const", "checker", "sparse", "ulp")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_sizes.json")


def make_image(recipe, seed, h, w):
    """(h, w, 3) uint8 — or float32 in [0, 1] for "ulp" — from a recipe name and a seed."""
    rng = np.random.default_rng(seed)
    if recipe == "noise":                                   # incompressible: long codes, stuffed bytes
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if recipe == "smooth":                                  # gradient + low noise: short runs, small categories
        ramp = np.add.outer(np.arange(h) * (200.0 / h), np.arange(w) * (55.0 / w))[..., None] * np.array([1.0, 0.8, 0.6])
        return np.clip(ramp + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    if recipe == "const":                                   # every DC difference after the first 0, every block EOB-only
        return np.full((h, w, 3), int(rng.integers(0, 256)), np.uint8)
    if recipe == "checker":                                 # 0 / 255 at pixel pitch: the largest coefficients
        return np.broadcast_to((np.add.outer(np.arange(h), np.arange(w)) % 2 * 255).astype(np.uint8)[..., None], (h, w, 3)).copy()
    if recipe == "sparse":                                  # one high-frequency coefficient per luminance block: zero runs >= 16 -> ZRL
        x = np.arange(8)
        img = np.empty((h, w), np.float64)
        for by in range(h // 8):
            for bx in range(w // 8):
                u, v = int(rng.integers(5, 8)), int(rng.integers(5, 8))
                amp = float(rng.integers(60, 120))
                img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = 128 + amp * np.outer(np.cos((2 * x + 1) * u * np.pi / 16), np.cos((2 * x + 1) * v * np.pi / 16))
        return np.repeat(np.clip(np.rint(img), 0, 255).astype(np.uint8)[..., None], 3, axis=2)
    if recipe == "ulp":                                     # float32 within one ulp of k / 255: the truncation (x * 255).astype(uint8) decides
        k = rng.integers(0, 256, (h, w, 3))
        x = (k / 255.0).astype(np.float32)
        step = rng.integers(-1, 2, (h, w, 3))
        x = np.where(step < 0, np.nextafter(x, np.float32(-1)), np.where(step > 0, np.nextafter(x, np.float32(2)), x)).astype(np.float32)
        return np.clip(x, np.float32(0), np.float32(1))
    raise KeyError(recipe)


def to_u8(img):
    """The reward's truncation of float images (callbacks.encode_jpeg)."""
    return img if img.dtype == np.uint8 else (img * 255).astype(np.uint8)


def load_golden():
    with open(GOLDEN) as f:
        return {(c["recipe"], c["seed"], c["h"], c["w"], c["quality"]): c["bytes"] for c in json.load(f)["cases"]}


# ------------------------------------------------------------------------------------------------ stream parser
def parse_jpeg(data):
    """Facts about a baseline JPEG file `data` (bytes): `segments` [(marker, length incl. the 2 length bytes)], `header_bytes` (everything before the
    entropy-coded data), `sampling` (the SOF0 sampling bytes), `dht_lengths`, `scans`, `restart_markers`, `stuffed` (0xFF00 pairs in the scan), `bits`
    (bits the scan's symbols take), `pad_ok` (the rest of the last byte is 1-bits), `zrl` (ZRL symbols), `eob`, `max_ac_size`, `max_dc_size`."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    pos, segments, tables, sampling, dht_lengths, scans = 2, [], {}, None, [], 0
    comps, scan_tables = [], {}
    while True:
        assert data[pos] == 0xFF
        marker, length = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        body = data[pos + 4:pos + 2 + length]
        segments.append((marker, length))
        if marker == 0xC4:                                  # DHT (one table per segment is what the encoder writes; several are parsed anyway)
            dht_lengths.append(length + 2)
            q = 0
            while q < len(body):
                tc_th, counts = body[q], body[q + 1:q + 17]
                vals = body[q + 17:q + 17 + sum(counts)]
                q += 17 + sum(counts)
                table, code, k = {}, 0, 0
                for ln in range(1, 17):
                    for _ in range(counts[ln - 1]):
                        table[(ln, code)] = vals[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                tables[tc_th] = table
        elif marker == 0xC0:                                # SOF0
            height, width, nc = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            comps = [(body[6 + 3 * i], body[7 + 3 * i]) for i in range(nc)]
            sampling = tuple(c[1] for c in comps)
        elif marker == 0xDA:                                # SOS: the entropy-coded segment follows
            scans += 1
            ns = body[0]
            for i in range(ns):
                scan_tables[body[1 + 2 * i]] = (body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15)
            pos += 2 + length
            break
        pos += 2 + length
    header_bytes = pos
    ecs = data[pos:-2]
    restart = sum(1 for i in range(len(ecs) - 1) if ecs[i] == 0xFF and 0xD0 <= ecs[i + 1] <= 0xD7)
    stuffed = ecs.count(b"\xff\x00")
    raw = ecs.replace(b"\xff\x00", b"\xff")
    assert len(raw) + stuffed == len(ecs)
    bits = "".join(f"{b:08b}" for b in raw)
    p = 0
    stats = dict(zrl=0, eob=0, max_ac_size=0, max_dc_size=0)

    def symbol(table):
        nonlocal p
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | (bits[p] == "1")
            p += 1
            if (ln, code) in table:
                return table[(ln, code)]
        raise AssertionError("bad Huffman code")

    def block(cid):
        nonlocal p
        td, ta = scan_tables[cid]
        s = symbol(tables[td])
        stats["max_dc_size"] = max(stats["max_dc_size"], s)
        p += s
        k = 1
        while k < 64:
            rs = symbol(tables[0x10 | ta])
            r, s = rs >> 4, rs & 15
            if s == 0:
                if r == 15:
                    stats["zrl"] += 1
                    k += 16
                    continue
                stats["eob"] += 1
                break
            stats["max_ac_size"] = max(stats["max_ac_size"], s)
            k += r + 1
            p += s

    hmax, vmax = max(c[1] >> 4 for c in comps), max(c[1] & 15 for c in comps)
    mcus = -(-width // (8 * hmax)) * -(-height // (8 * vmax))
    for _ in range(mcus):
        for cid, hv in comps:
            for _ in range((hv >> 4) * (hv & 15)):
                block(cid)
    assert len(bits) - p < 8, "scan data longer than its symbols"
    return dict(segments=segments, header_bytes=header_bytes, sampling=sampling, dht_lengths=dht_lengths, scans=scans, restart_markers=restart,
                stuffed=stuffed, bits=p, pad_ok=set(bits[p:]) <= {"1"}, **stats)
