"""HF TinyLlama checkpoint -> .gten file.

Counterpart of the reference's `tinyllama_to_gten.py` (behaviour restated, nothing copied):
  * record order and framing: tinyllama_to_gten.py:94-109,150-201 / reader tinyllama.cpp:301-392
  * weight quantizers: tinyllama_to_gten.py:24-91 -- per 32-wide block delta32 = absmax / 127 (Q8) or / 7 (Q4),
    q = round-half-to-EVEN(x / delta32) (torch.round), stored delta = fp16(delta32); Q4 adds 7 and packs elements
    0..15 into the high nibbles, 16..31 into the low nibbles; a zero block stores delta 0 and q 0
  * norm vectors stay fp16 in every mode; embedding and lm_head are quantized like any linear

Checkpoint dtype: the reference divides absmax by 127 (7) IN THE CHECKPOINT'S OWN DTYPE before the delta goes to f32
(tinyllama_to_gten.py:38-39, 68-69), so for a bf16 checkpoint -- TinyLlama's own -- the f32 delta is a bf16 value, and
the quants follow from it.  `quantize_q8 / quantize_q4(w, src=...)` reproduce that for src in ("f32", "bf16", "f16");
`open_checkpoint` reads bf16 / f16 / f32 safetensors (through torch for bf16, which numpy cannot hold) and reports each
tensor's dtype.  Other dtypes are refused.

numpy only (plus `safetensors`, and torch for bf16 files, to read a checkpoint); pinned byte for byte by tests/golden/converter_pins.npz
(tests/test_convert_cpu.py).  The GPU library repacks these blocks at load (gten_hip_pack_weight).

    python -m tinyllama.cpp_amd.convert <model.safetensors | checkpoint dir> out.q4.gten --dtype q4
"""
import os
import struct
import sys

import numpy as np

GTEN_MAGIC = 0x454C49464E455447
DTYPES = ("f16", "q8", "q4")


def to_f16(w):
    return np.ascontiguousarray(w, dtype=np.float32).astype(np.float16).view(np.uint8).reshape(w.shape[0], -1)


def _blocks(w):
    w = np.ascontiguousarray(w, dtype=np.float32)
    rows, cols = w.shape
    if cols % 32:
        raise ValueError(f"row length {cols} is not a multiple of the 32-wide quant block")
    return w.reshape(rows, cols // 32, 32), rows, cols // 32


SRC_DTYPES = ("f32", "bf16", "f16")


def _round_to(x, src):
    """f32 values rounded (to nearest even) to the checkpoint's dtype, returned as f32"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if src == "f32":
        return x
    if src == "f16":
        return x.astype(np.float16).astype(np.float32)
    if src == "bf16":
        u = x.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000          # round to nearest even on the upper 16 bits
        return u.astype(np.uint32).view(np.float32)
    raise ValueError(f"checkpoint dtype {src!r} not in {SRC_DTYPES}")


def _quants(blocks, qmax, src="f32"):
    amax = np.abs(blocks).max(axis=2, keepdims=True)
    delta = _round_to((amax / np.float32(qmax)).astype(np.float32), src)   # the division happens in the checkpoint's dtype
    scale = np.divide(np.float32(1.0), delta, out=np.zeros_like(delta), where=delta != 0)
    q = np.rint(blocks * scale).astype(np.int32)          # np.rint: half to even, like torch.round
    return q, delta.astype(np.float16)


def quantize_q8(w, src="f32"):
    """[rows][cols] f32 -> [rows][cols/32 * 34] bytes: {f16 delta, int8 x 32} per block"""
    blocks, rows, nb = _blocks(w)
    q, d16 = _quants(blocks, 127, src)
    out = np.empty((rows, nb, 34), np.uint8)
    out[:, :, :2] = d16.view(np.uint8).reshape(rows, nb, 2)
    out[:, :, 2:] = q.astype(np.int8).view(np.uint8)
    return out.reshape(rows, nb * 34)


def quantize_q4(w, src="f32"):
    """[rows][cols] f32 -> [rows][cols/32 * 18] bytes: {f16 delta, 16 bytes: hi nibble = element j + 7, lo = element j + 16 + 7}"""
    blocks, rows, nb = _blocks(w)
    q, d16 = _quants(blocks, 7, src)
    q = (q + 7).astype(np.uint8)
    out = np.empty((rows, nb, 18), np.uint8)
    out[:, :, :2] = d16.view(np.uint8).reshape(rows, nb, 2)
    out[:, :, 2:] = (q[:, :, :16] << 4) | q[:, :, 16:]
    return out.reshape(rows, nb * 18)


def quantize(w, dtype, src="f32"):
    if dtype == "f16":
        return to_f16(w)
    return {"q8": quantize_q8, "q4": quantize_q4}[dtype](w, src)


def tensor_names(n_layers):
    """HF keys in .gten record order (tinyllama.cpp:345-391); second field: quantized like a linear?"""
    names = [("model.embed_tokens.weight", True)]
    for i in range(n_layers):
        p = f"model.layers.{i}."
        names += [(p + f"self_attn.{k}_proj.weight", True) for k in ("q", "k", "v", "o")]
        names += [(p + f"mlp.{k}_proj.weight", True) for k in ("gate", "up", "down")]
        names += [(p + "input_layernorm.weight", False), (p + "post_attention_layernorm.weight", False)]
    names += [("model.norm.weight", False), ("lm_head.weight", True)]
    return names


def write_gten(path, get_tensor, n_layers, dtype, progress=None):
    """get_tensor(name) -> 2-D (linear) or 1-D (norm) float array, or a pair (array, checkpoint dtype in SRC_DTYPES).
    Returns the number of bytes written."""
    if dtype not in DTYPES:
        raise ValueError(f"dtype {dtype!r} not in {DTYPES}")
    total = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<q", GTEN_MAGIC))
        total += 8
        for name, is_linear in tensor_names(n_layers):
            got = get_tensor(name)
            w, src = got if isinstance(got, tuple) else (got, "f32")
            w = np.asarray(w, dtype=np.float32)
            if is_linear:
                if w.ndim != 2:
                    raise ValueError(f"{name}: expected a matrix, got shape {w.shape}")
                payload = quantize(w, dtype, src)
            else:
                payload = to_f16(w.reshape(1, -1))
            raw = name.encode()
            # the reference writes every name twice (length + bytes), then the payload size
            for _ in range(2):
                f.write(struct.pack("<i", len(raw)))
                f.write(raw)
            buf = payload.tobytes()
            f.write(struct.pack("<i", len(buf)))
            f.write(buf)
            total += 2 * (4 + len(raw)) + 4 + len(buf)
            if progress:
                progress(name, payload.shape)
    return total


def open_checkpoint(src):
    """name -> (f32 array, checkpoint dtype) accessor over one .safetensors file or a directory of shards"""
    from safetensors import safe_open
    files = [src] if os.path.isfile(src) else sorted(os.path.join(src, f) for f in os.listdir(src) if f.endswith(".safetensors"))
    if not files:
        raise FileNotFoundError(f"no .safetensors under {src}")
    handles = [safe_open(f, framework="np") for f in files]
    index = {k: (h, f) for h, f in zip(handles, files) for k in h.keys()}
    pt_handles = {}

    def get(name):
        if name not in index:
            raise KeyError(f"{name} missing from the checkpoint")
        h, f = index[name]
        dt = h.get_slice(name).get_dtype()
        if dt in ("F32", "F16"):
            return np.asarray(h.get_tensor(name), dtype=np.float32), ("f32" if dt == "F32" else "f16")
        if dt == "BF16":
            import torch                       # numpy has no bf16: read through torch, hand on the exact f32 values
            if f not in pt_handles:
                pt_handles[f] = safe_open(f, framework="pt")
            return pt_handles[f].get_tensor(name).to(torch.float32).numpy(), "bf16"
        raise ValueError(f"{name}: checkpoint dtype {dt} is not supported (f32, f16 or bf16)")

    n_layers = 1 + max((int(k.split(".")[2]) for k in index if k.startswith("model.layers.")), default=-1)
    return get, n_layers


LORA_MAX_RANK = 64          # GTEN_HIP_LORA_MAX_RANK (include/gten_hip_lora.h)


def open_lora(path, n_layers=None):
    """A PEFT LoRA adapter (a directory with adapter_model.safetensors + adapter_config.json, or the .safetensors file beside
    its config) -> ({hf weight name: (A [r][cols], B [rows][r])}, scale) for HostModel.load_checkpoint.  A and B keep the file's
    dtype: float32, float16, or bf16 as raw uint16 words.  scale = lora_alpha / r, or / sqrt(r) with use_rslora.  Device-free.
    What the merge on the device (include/gten_hip_lora.h) cannot honour is refused by name."""
    import json
    from safetensors import safe_open
    d = path if os.path.isdir(path) else os.path.dirname(os.path.abspath(path))
    file = os.path.join(d, "adapter_model.safetensors") if os.path.isdir(path) else path
    with open(os.path.join(d, "adapter_config.json")) as f:
        cfg = json.load(f)
    r, alpha = int(cfg["r"]), float(cfg.get("lora_alpha", cfg["r"]))
    refusals = [(cfg.get("use_dora"), "DoRA (use_dora)"), (cfg.get("bias", "none") != "none", f"bias terms (bias = {cfg.get('bias')!r})"),
                (cfg.get("modules_to_save"), f"modules_to_save {cfg.get('modules_to_save')}"),
                (cfg.get("rank_pattern") or cfg.get("alpha_pattern"), "a rank_pattern / alpha_pattern (one rank and scale per adapter)"),
                (not 1 <= r <= LORA_MAX_RANK, f"rank {r} outside 1..{LORA_MAX_RANK}")]
    for hit, what in refusals:
        if hit:
            raise ValueError(f"{path}: the adapter has {what}, which cannot be merged on the device")
    scale = alpha / (r ** 0.5 if cfg.get("use_rslora") else r)
    linear = None if n_layers is None else {n for n, lin in tensor_names(n_layers)[1:-1] if lin}
    parts = {}
    with safe_open(file, framework="np") as h_np:
        pt = None
        for key in h_np.keys():
            if "lora_embedding_" in key:
                raise ValueError(f"{path}: {key} is an embedding adapter, which cannot be merged on the device")
            if "lora_magnitude_vector" in key:
                raise ValueError(f"{path}: {key} is a DoRA magnitude, which cannot be merged on the device")
            head, _, tail = key.partition(".lora_")
            if not key.startswith("base_model.model.") or tail not in ("A.weight", "B.weight"):
                raise ValueError(f"{path}: {key} is not a lora_A / lora_B weight of a linear layer")
            name = head[len("base_model.model."):] + ".weight"
            if "embed_tokens" in name or name.startswith("lm_head") or (linear is not None and name not in linear):
                raise ValueError(f"{path}: {key} adapts {name}, which takes no adapter (only q, k, v, o, gate, up, down of a block)")
            dt = h_np.get_slice(key).get_dtype()
            if dt in ("F32", "F16"):
                m = np.ascontiguousarray(h_np.get_tensor(key))
            elif dt == "BF16":
                import torch                   # numpy has no bf16: the raw words through torch
                pt = pt or safe_open(file, framework="pt")
                m = pt.get_tensor(key).contiguous().view(torch.int16).numpy().view(np.uint16)
            else:
                raise ValueError(f"{path}: {key} has dtype {dt} (f32, f16 or bf16)")
            parts.setdefault(name, {})[tail[0]] = m
    out = {}
    for name, p in parts.items():
        if set(p) != {"A", "B"} or p["A"].dtype != p["B"].dtype or p["A"].shape[0] != r or p["B"].shape[1] != r:
            raise ValueError(f"{path}: {name} needs lora_A [{r}][cols] and lora_B [rows][{r}] of one dtype")
        out[name] = (p["A"], p["B"])
    return out, scale


# ggml type code -> (name, bytes of a block, elements of a block): what include/gten_hip_gguf.h decodes, and the dense types
GGML_TYPES = {0: ("F32", 4, 1), 1: ("F16", 2, 1), 30: ("BF16", 2, 1), 2: ("Q4_0", 18, 32), 6: ("Q5_0", 22, 32), 8: ("Q8_0", 34, 32),
              12: ("Q4_K", 144, 256), 13: ("Q5_K", 176, 256), 14: ("Q6_K", 210, 256)}
GGML_DENSE = {0: "f32", 1: "f16", 30: "bf16"}
_GGUF_SCALARS = {0: "<B", 1: "<b", 2: "<H", 3: "<h", 4: "<I", 5: "<i", 6: "<f", 7: "<?", 10: "<Q", 11: "<q", 12: "<d"}
_GGUF_BLOCK = {"attn_q": "self_attn.q_proj", "attn_k": "self_attn.k_proj", "attn_v": "self_attn.v_proj", "attn_output": "self_attn.o_proj",
               "ffn_gate": "mlp.gate_proj", "ffn_up": "mlp.up_proj", "ffn_down": "mlp.down_proj", "attn_norm": "input_layernorm",
               "ffn_norm": "post_attention_layernorm"}


def gguf_row_map(rows, n_head):
    """source row of every destination row of attn_q / attn_k (include/gten_hip_gguf.h): llama.cpp's converter interleaves the
    two halves of a head's rows; n_head 0: the identity"""
    r = np.arange(rows)
    if not n_head:
        return r
    d = rows // n_head
    return r // d * d + 2 * (r % d % (d // 2)) + r % d // (d // 2)


def _gguf_hf_name(name):
    """a llama-family GGUF tensor name -> the key of tensor_names, or None"""
    fixed = {"token_embd.weight": "model.embed_tokens.weight", "output_norm.weight": "model.norm.weight", "output.weight": "lm_head.weight"}
    if name in fixed:
        return fixed[name]
    part = name.split(".")
    if len(part) == 4 and part[0] == "blk" and part[1].isdigit() and part[2] in _GGUF_BLOCK and part[3] == "weight":
        return f"model.layers.{int(part[1])}.{_GGUF_BLOCK[part[2]]}.weight"
    return None


class GgufFile:
    """open_gguf's accessor: `tensors` maps a tensor_names key to (memory-mapped block bytes uint8[], ggml type, rows, cols) -- a
    vector has rows 1 --, `meta` holds every scalar and string key, and n_layers / n_head / n_head_kv / alignment what the loader needs"""

    def __init__(self, path, tensors, meta, alignment):
        self.path, self.tensors, self.meta, self.alignment = path, tensors, meta, alignment
        self.n_layers = int(meta["llama.block_count"])
        self.n_head = int(meta["llama.attention.head_count"])
        self.n_head_kv = int(meta.get("llama.attention.head_count_kv", self.n_head))

    def __getitem__(self, name):
        return self.tensors[name]


def open_gguf(path):
    """A llama-family GGUF file (version 2 or 3, little-endian) -> GgufFile.  Device-free and hand-written: the header, the
    key / value section (all 13 value types; arrays are skipped), the tensor infos, the data section at `general.alignment`.
    Tensors are NOT dequantised: their bytes stay in the file's mapping, as HostModel.load_gguf uploads them.  A file without
    output.weight gets token_embd's bytes as lm_head.  What cannot be loaded is refused by name."""
    raw = np.memmap(path, np.uint8, "r")
    at = 0

    def take(fmt):
        nonlocal at
        if at + struct.calcsize(fmt) > raw.size:
            raise ValueError(f"{path}: the file ends inside its header")
        v = struct.unpack_from(fmt, raw, at)
        at += struct.calcsize(fmt)
        return v if len(v) > 1 else v[0]

    def string():
        nonlocal at
        n = take("<Q")
        if at + n > raw.size:
            raise ValueError(f"{path}: the file ends inside its header")
        s = bytes(raw[at:at + n]).decode("utf-8", "replace")
        at += n
        return s

    def value(vt, keep=True):
        nonlocal at
        if vt in _GGUF_SCALARS:
            return take(_GGUF_SCALARS[vt])
        if vt == 8:
            return string()
        if vt == 9:
            et, n = take("<IQ")
            if et in _GGUF_SCALARS:
                at += n * struct.calcsize(_GGUF_SCALARS[et])
            else:
                for _ in range(n):
                    value(et, False)
            return None
        raise ValueError(f"{path}: key / value type {vt} is not a GGUF value type")

    if raw.size < 24 or bytes(raw[:4]) != b"GGUF":
        raise ValueError(f"{path}: not a GGUF file (magic {bytes(raw[:4])!r})")
    at = 4
    version = take("<I")
    if version not in (2, 3):
        if version & 0xFFFF == 0 and version >> 24 in (1, 2, 3):
            raise ValueError(f"{path}: a big-endian GGUF file (version field {version:#010x}); only little-endian files are read")
        raise ValueError(f"{path}: GGUF version {version} is not supported (2 or 3)")
    n_tensors, n_kv = take("<QQ")
    meta = {}
    for _ in range(n_kv):
        key = string()
        v = value(take("<I"))
        if v is not None:
            meta[key] = v
    alignment = int(meta.get("general.alignment", 32))
    infos = []
    for _ in range(n_tensors):
        name = string()
        n_dims = take("<I")
        ne = [take("<Q") for _ in range(n_dims)]
        code, offset = take("<IQ")
        infos.append((name, ne, code, offset))
    data0 = -(-at // alignment) * alignment
    tensors = {}
    for name, ne, code, offset in infos:
        hf = _gguf_hf_name(name)
        if hf is None:
            continue                                              # (rope_freqs and the like: nothing this model reads)
        if code not in GGML_TYPES:
            raise ValueError(f"{path}: {name} has ggml type {code}, which is not supported ({', '.join(f'{n} {c}' for c, (n, _, _) in sorted(GGML_TYPES.items()))})")
        if len(ne) not in (1, 2) or offset % alignment:
            raise ValueError(f"{path}: {name} has the wrong shape {ne} or an offset {offset} off the alignment {alignment}")
        _, unit, elems = GGML_TYPES[code]
        cols, rows = ne[0], (ne[1] if len(ne) == 2 else 1)
        if cols % elems:
            raise ValueError(f"{path}: {name} has the wrong shape: {cols} columns are no multiple of the {elems} elements of a block of ggml type {code}")
        nbytes = rows * (cols // elems) * unit
        if data0 + offset + nbytes > raw.size:
            raise ValueError(f"{path}: {name} ends behind the file")
        tensors[hf] = (raw[data0 + offset:data0 + offset + nbytes], code, rows, cols)
    for key in ("llama.block_count", "llama.attention.head_count"):
        if key not in meta:
            raise ValueError(f"{path}: the key {key} is missing")
    if "lm_head.weight" not in tensors and "model.embed_tokens.weight" in tensors:
        tensors["lm_head.weight"] = tensors["model.embed_tokens.weight"]
    back = {v: k for k, v in _GGUF_BLOCK.items()}
    for hf, _ in tensor_names(int(meta["llama.block_count"])):
        if hf not in tensors:
            p = hf.split(".")
            gg = f"blk.{p[2]}.{back['.'.join(p[3:-1])]}.weight" if p[1] == "layers" else {"model.embed_tokens.weight": "token_embd.weight", "model.norm.weight": "output_norm.weight"}.get(hf, "output.weight")
            raise ValueError(f"{path}: the tensor {gg} is missing")
    return GgufFile(path, tensors, meta, alignment)


W4_LINEARS = tuple(f"self_attn.{k}_proj" for k in ("q", "k", "v", "o")) + tuple(f"mlp.{k}_proj" for k in ("gate", "up", "down"))


class QuantizedCheckpoint:
    """open_quantized's accessor.  layout "gptq" | "awq", zero_offset, group_size (-1: one group), n_layers and `config` (the
    quantisation settings as read); linear(name) / dense(name) take a tensor_names key; trivial_g_idx maps every linear that has
    a g_idx to whether it equals k / group_size (linear() then hands None on, the device's fast form)."""

    def __init__(self, src, get, n_layers, layout, zero_offset, group_size, config, raw):
        self.src, self._get, self.n_layers, self.layout, self.zero_offset, self.group_size = src, get, n_layers, layout, zero_offset, group_size
        self.config, self._raw, self.trivial_g_idx = config, raw, {}

    def is_quantized(self, name):
        return name.startswith("model.layers.") and name[:-len(".weight")].split(".", 3)[3] in W4_LINEARS

    def dense(self, name):
        """(f32 array, checkpoint dtype) of embed_tokens, lm_head or a norm vector"""
        return self._get(name)

    def linear(self, name):
        """(qweight int32, qzeros int32, scales f16, g_idx int32 or None, rows N, cols K) of a block linear, shapes checked"""
        base = name[:-len(".weight")]
        qweight, qzeros, scales = (self._raw(f"{base}.{part}") for part in ("qweight", "qzeros", "scales"))
        if qweight.ndim != 2 or qweight.dtype != np.int32 or qzeros.dtype != np.int32 or scales.dtype != np.float16:
            raise ValueError(f"{self.src}: {base} needs int32 qweight and qzeros matrices and float16 scales")
        rows, cols = (qweight.shape[1], qweight.shape[0] * 8) if self.layout == "gptq" else (qweight.shape[1] * 8, qweight.shape[0])
        gs = self.group_size
        if cols % 32 or rows % 8 or (gs != -1 and cols % gs):
            raise ValueError(f"{self.src}: {base} has the wrong shape: {rows} x {cols} with group_size {gs} (cols % 32, rows % 8, cols % group_size)")
        groups = 1 if gs == -1 else cols // gs
        if qzeros.shape != (groups, rows // 8) or scales.shape != (groups, rows):
            raise ValueError(f"{self.src}: {base} has the wrong shape: qzeros {qzeros.shape} and scales {scales.shape} for {groups} groups of a {rows} x {cols} weight")
        g_idx = None
        if self.layout == "gptq" and self._raw(f"{base}.g_idx", missing_ok=True) is not None:
            g_idx = np.ascontiguousarray(self._raw(f"{base}.g_idx"), dtype=np.int32)
            if g_idx.shape != (cols,):
                raise ValueError(f"{self.src}: {base}.g_idx has the wrong shape {g_idx.shape} for {cols} input features")
            self.trivial_g_idx[name] = bool(np.array_equal(g_idx, np.arange(cols) // (cols if gs == -1 else gs)))
            if self.trivial_g_idx[name]:
                g_idx = None
        return qweight, qzeros, scales, g_idx, rows, cols


def open_quantized(src):
    """A GPTQ or AWQ 4-bit Hugging Face checkpoint -- one .safetensors file or a directory of them, with `quantization_config` in
    config.json or a quantize_config.json beside it -> QuantizedCheckpoint for HostModel.load_quantized.  Device-free; nothing is
    dequantised.  Accepted: quant_method gptq (checkpoint_format gptq | gptq_v2; desc_act and sym either way) and awq (version
    gemm).  What include/gten_hip_w4.h cannot take is refused by name."""
    import json
    from safetensors import safe_open
    d = src if os.path.isdir(src) else os.path.dirname(os.path.abspath(src))
    cfg = None
    if os.path.exists(os.path.join(d, "config.json")):
        with open(os.path.join(d, "config.json")) as f:
            cfg = json.load(f).get("quantization_config")
    if cfg is None and os.path.exists(os.path.join(d, "quantize_config.json")):
        with open(os.path.join(d, "quantize_config.json")) as f:
            cfg = json.load(f)
    if cfg is None:
        raise ValueError(f"{src}: no quantization_config in config.json and no quantize_config.json beside the checkpoint")
    method = str(cfg.get("quant_method", "gptq")).lower()
    bits, gs = int(cfg.get("bits", cfg.get("w_bit", 0))), int(cfg.get("group_size", cfg.get("q_group_size", 0)))
    if method not in ("gptq", "awq"):
        raise ValueError(f"{src}: quant_method {method!r} is not supported (gptq or awq)")
    if bits != 4:
        raise ValueError(f"{src}: {bits}-bit weights are not supported (4 bits only)")
    if gs != -1 and (gs < 32 or gs % 32):
        raise ValueError(f"{src}: group_size {gs} is not supported (-1, or a multiple of 32 that divides the input features)")
    if method == "gptq":
        fmt = str(cfg.get("checkpoint_format", "gptq")).lower()
        if cfg.get("is_marlin_format") or fmt not in ("gptq", "gptq_v2"):
            raise ValueError(f"{src}: GPTQ checkpoint_format {'marlin' if cfg.get('is_marlin_format') else fmt!r} is a repacked form (Marlin, exllama) "
                             "that is not supported (gptq or gptq_v2)")
        zero_offset = 1 if fmt == "gptq" else 0
    else:
        version = str(cfg.get("version", "gemm")).lower()
        if version != "gemm":
            raise ValueError(f"{src}: AWQ version {version!r} is not supported (gemm only; not gemv, gemv_fast, marlin or exllama)")
        if not cfg.get("zero_point", True):
            raise ValueError(f"{src}: AWQ without zero points (zero_point false) is not supported")
        zero_offset = 0
    get, n_layers = open_checkpoint(src)
    files = [src] if os.path.isfile(src) else sorted(os.path.join(src, f) for f in os.listdir(src) if f.endswith(".safetensors"))
    handles = [safe_open(f, framework="np") for f in files]
    index = {k: h for h in handles for k in h.keys()}

    def raw(key, missing_ok=False):
        if key not in index:
            if missing_ok:
                return None
            raise ValueError(f"{src}: the tensor {key} is missing")
        return index[key].get_tensor(key)

    ck = QuantizedCheckpoint(src, get, n_layers, method, zero_offset, gs, dict(cfg), raw)
    for name, _ in tensor_names(n_layers):
        keys = [f"{name[:-len('.weight')]}.{part}" for part in ("qweight", "qzeros", "scales")] if ck.is_quantized(name) else [name]
        for key in keys:
            if key not in index:
                raise ValueError(f"{src}: the tensor {key} is missing")
    return ck


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src")
    ap.add_argument("out")
    ap.add_argument("--dtype", choices=DTYPES, default="q4")
    a = ap.parse_args(argv)
    get, n_layers = open_checkpoint(a.src)
    n = write_gten(a.out, get, n_layers, a.dtype, progress=lambda name, shape: print(f"  {name:56s} {shape}", file=sys.stderr))
    print(f"{a.out}: {n} bytes, {n_layers} layers, {a.dtype}")


if __name__ == "__main__":
    main()
