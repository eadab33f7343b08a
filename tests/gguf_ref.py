"""ggml's dequantisation of the six block formats include/gten_hip_gguf.h decodes, restated in NumPy f32 (every product and
difference one rounded f32 operation, in the header's order), random block streams for them, the row map, and a minimal GGUF
writer.  What tests/test_gguf_gpu.py and tests/test_gguf_cpu.py compare against."""
import struct

import numpy as np

F32 = np.float32
# ggml type code -> (name, bytes of a block, elements of a block)
FORMATS = {8: ("Q8_0", 34, 32), 2: ("Q4_0", 18, 32), 6: ("Q5_0", 22, 32), 12: ("Q4_K", 144, 256), 13: ("Q5_K", 176, 256), 14: ("Q6_K", 210, 256)}


def src_bytes(code, rows, cols):
    _, unit, elems = FORMATS[code]
    return rows * (cols // elems) * unit


def _f16(b, at):
    """the f16 at byte `at` of every block, widened to f32: [n][1]"""
    return np.ascontiguousarray(b[:, at:at + 2]).view(np.float16).astype(F32)


def _k_scales(sc):
    """the 6-bit (scale, min) pairs of Q4_K / Q5_K: u8 [n][12] -> two f32 [n][8]"""
    sc = sc.astype(np.uint32)
    s = np.concatenate([sc[:, 0:4] & 63, (sc[:, 8:12] & 15) | ((sc[:, 0:4] >> 6) << 4)], axis=1)
    m = np.concatenate([sc[:, 4:8] & 63, (sc[:, 8:12] >> 4) | ((sc[:, 4:8] >> 6) << 4)], axis=1)
    return s.astype(F32), m.astype(F32)


def dequant(stream, code, rows, cols):
    """uint8 block stream of a [rows][cols] tensor of ggml type `code` -> f32 [rows][cols]"""
    _, unit, elems = FORMATS[code]
    b = np.frombuffer(bytes(stream), np.uint8).reshape(-1, unit)
    assert len(b) == rows * (cols // elems)
    lo, hi = (lambda q: (q & 15).astype(np.int32)), (lambda q: (q >> 4).astype(np.int32))
    with np.errstate(over="ignore", invalid="ignore"):
        if code == 8:
            x = b[:, 2:].view(np.int8).astype(F32) * _f16(b, 0)
        elif code == 2:
            x = np.concatenate([lo(b[:, 2:]) - 8, hi(b[:, 2:]) - 8], axis=1).astype(F32) * _f16(b, 0)
        elif code == 6:
            qh = np.ascontiguousarray(b[:, 2:6]).view(np.uint32)
            bit = ((qh >> np.arange(32, dtype=np.uint32)) & 1).astype(np.int32) << 4
            x = (np.concatenate([lo(b[:, 6:]), hi(b[:, 6:])], axis=1) | bit) - 16
            x = x.astype(F32) * _f16(b, 0)
        elif code in (12, 13):
            s, m = _k_scales(b[:, 4:16])
            qs = b[:, (16 if code == 12 else 48):].reshape(-1, 4, 32)
            q = np.stack([lo(qs), hi(qs)], axis=2).reshape(-1, 8, 32)               # sub-block 2 g + h
            if code == 13:
                q = q + ((((b[:, 16:48].astype(np.int32)[:, None, :] >> np.arange(8)[None, :, None]) & 1)) << 4)
            t = (_f16(b, 0) * s)[:, :, None]
            x = t * q.astype(F32) - (_f16(b, 2) * m)[:, :, None]
        else:
            ql, qh = b[:, :128].reshape(-1, 2, 2, 32), b[:, 128:192].reshape(-1, 2, 1, 32).astype(np.int32)
            low = np.stack([lo(ql), hi(ql)], axis=2).reshape(-1, 2, 4, 32)          # k = 2 (nibble) + (k & 1)
            q = (low | (((qh >> (2 * np.arange(4))[None, None, :, None]) & 3) << 4)) - 32
            t = _f16(b, 208) * b[:, 192:208].view(np.int8).astype(F32)              # [n][16]: sc[8 n + 2 k + l / 16]
            x = np.repeat(t, 16, axis=1).reshape(-1, 2, 4, 32) * q.astype(F32)
    return np.ascontiguousarray(x, dtype=F32).reshape(rows, cols)


def row_map(rows, n_head):
    """source row of every destination row (include/gten_hip_gguf.h)"""
    r = np.arange(rows)
    if not n_head:
        return r
    D = rows // n_head
    h, rem = r // D, r % D
    return h * D + 2 * (rem % (D // 2)) + rem // (D // 2)


def random_stream(code, rows, cols, rng, d_max=0.05):
    """every quant, high-bit and scale byte uniform; d and dmin finite f16 in (-d_max, d_max): all products stay far from f32's limits"""
    _, unit, elems = FORMATS[code]
    b = rng.integers(0, 256, (rows * (cols // elems), unit), dtype=np.uint8)
    for at in {8: (0,), 2: (0,), 6: (0,), 12: (0, 2), 13: (0, 2), 14: (208,)}[code]:
        b[:, at:at + 2] = rng.uniform(-d_max, d_max, (len(b), 1)).astype(np.float16).view(np.uint8)
    return b.reshape(-1)


def _gstr(s):
    return struct.pack("<Q", len(s)) + s.encode()


def write_gguf(path, tensors, kv, alignment=32, version=3, magic=b"GGUF"):
    """tensors: [(name, ggml type, (rows, cols) or (n,), bytes)]; kv: {key: u32 value}.  The header, the keys (general.alignment
    first when it is not 32), the tensor infos, then each tensor's bytes at the next multiple of `alignment`."""
    kv = dict(kv, **({"general.alignment": alignment} if alignment != 32 else {}))
    out = magic + struct.pack("<IQQ", version, len(tensors), len(kv))
    for k, v in kv.items():
        out += _gstr(k) + struct.pack("<II", 4, v)
    at, data = 0, b""
    for name, code, shape, raw in tensors:
        out += _gstr(name) + struct.pack("<I", len(shape)) + b"".join(struct.pack("<Q", n) for n in reversed(shape)) + struct.pack("<IQ", code, at)
        data += bytes(raw) + b"\0" * (-len(raw) % alignment)
        at = len(data)
    with open(path, "wb") as f:
        f.write(out + b"\0" * (-len(out) % alignment) + data)
