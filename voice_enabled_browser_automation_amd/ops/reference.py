"""Plain-PyTorch (f32 math) reference implementations of every kernel in csrc/kernels.

Used on CPU tensors (tests, the CPU config) and as the numerics oracle for the HIP kernels.
Semantics (layouts, permutations, epilogues) match the kernels exactly.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F


def _rms_scale(xf: torch.Tensor, eps: float) -> torch.Tensor:
    return torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)


def linear(x, w, bias=None, *, out, residual=None, act="none", fuse_rms=False, eps=1e-5):
    xf = x.float()
    if fuse_rms:
        xf = xf * _rms_scale(xf, eps)
    y = xf @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    if act == "gelu":
        y = F.gelu(y)
    if residual is not None:
        y = y + residual.float()
    out.copy_(y.to(out.dtype))
    return out


def linear_swiglu(x, w_gu, *, fuse_rms=False, eps=1e-5, out):
    xf = x.float()
    if fuse_rms:
        xf = xf * _rms_scale(xf, eps)
    gu = xf @ w_gu.float().t()
    M, F2 = gu.shape
    t = gu.view(M, F2 // 32, 2, 16)
    h = F.silu(t[:, :, 0, :]) * t[:, :, 1, :]
    out.copy_(h.reshape(M, F2 // 2).to(out.dtype))
    return out


def _apply_rope(x: torch.Tensor, positions: torch.Tensor, rope: torch.Tensor) -> torch.Tensor:
    # x [M, H, D] natural layout; rotate-half convention
    D = x.shape[-1]
    half = D // 2
    cs = rope[positions.long()]  # [M, half, 2]
    c = cs[..., 0][:, None, :]
    s = cs[..., 1][:, None, :]
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def write_kv(k: torch.Tensor, v: torch.Tensor, slots: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor):
    bs = k_cache.shape[2]
    for m in range(k.shape[0]):
        s = int(slots[m])
        if s < 0:
            continue
        b, o = divmod(s, bs)
        k_cache[b, :, o, :] = k[m].to(k_cache.dtype)
        v_cache[b, :, o, :] = v[m].to(v_cache.dtype)


def qkv_rope_write(x, w_qkv, bias, *, fuse_rms, eps, n_q_heads, n_kv_heads, head_dim, rope, positions, slots, q_out,
                   k_cache, v_cache):
    from . import unpermute_qkv_cols

    M = x.shape[0]
    xf = x.float()
    if fuse_rms:
        xf = xf * _rms_scale(xf, eps)
    y = xf @ w_qkv.float().t()
    if bias is not None:
        y = y + bias.float()
    H = n_q_heads + 2 * n_kv_heads
    y = unpermute_qkv_cols(y, H, head_dim).view(M, H, head_dim)
    q, k, v = y[:, :n_q_heads], y[:, n_q_heads : n_q_heads + n_kv_heads], y[:, n_q_heads + n_kv_heads :]
    if rope is not None:
        q = _apply_rope(q, positions[:M], rope)
        k = _apply_rope(k, positions[:M], rope)
    # kernels round to bf16 before storing; mimic
    q_out[:M] = q.reshape(M, -1).to(q_out.dtype)
    write_kv(k, v, slots[:M], k_cache, v_cache)


def rmsnorm(x, w, *, eps=1e-5, residual=None, residual_out=None, out):
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
        residual_out.copy_(xf.to(residual_out.dtype))
    y = xf * _rms_scale(xf, eps)
    if w is not None:
        y = y * w.float()
    out.copy_(y.to(out.dtype))
    return out


def layernorm(x, w, b, *, eps=1e-5, residual=None, residual_out=None, out):
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
        residual_out.copy_(xf.to(residual_out.dtype))
    y = F.layer_norm(xf, (xf.shape[-1],), w.float(), b.float(), eps)
    out.copy_(y.to(out.dtype))
    return out


def embedding(ids, table, *, pos_table=None, positions=None, vocab_start=0, out):
    n = out.shape[0]
    idl = ids[:n].long() - vocab_start
    valid = (idl >= 0) & (idl < table.shape[0])
    e = table[idl.clamp(0, table.shape[0] - 1)].float() * valid[:, None].float()
    if pos_table is not None:
        e = e + pos_table[positions[:n].long()].float()
    out.copy_(e.to(out.dtype))
    return out


def _flat(x):
    """The whole storage of x as a 1-D view (strided views: offsets are relative to x's first element)."""
    n_el = x.untyped_storage().nbytes() // x.element_size()
    return x.as_strided((n_el,), (1,), 0)[x.storage_offset():]


def _gather_kv_heads(kv, seq: int, n: int, heads: int):
    """K, V [heads, n, D] (f32) for tokens 0..n-1 of table row `seq`, every kv head at once: the
    cache storage viewed as [blocks, heads, block_size, D] (the layout's strides), the sequence's
    blocks picked with one index_select."""
    bs = kv.block_size
    D = kv.k.shape[-1]
    nb = (n + bs - 1) // bs
    blk = kv.table[seq][:nb].long()

    def g(x):
        n_el = x.untyped_storage().nbytes() // x.element_size() - x.storage_offset()
        nblocks = (n_el - (heads - 1) * kv.sh - (bs - 1) * kv.st - D) // kv.sb + 1
        v = x.as_strided((nblocks, heads, bs, D), (kv.sb, kv.sh, kv.st, 1), x.storage_offset())
        return v.index_select(0, blk).permute(1, 0, 2, 3).reshape(heads, nb * bs, D)[:, :n].float()

    return g(kv.k), g(kv.v)


def decode_attention(q, kv, ctx_lens, seq_ids, *, n_q_heads, n_kv_heads, head_dim, scale, out):
    """Per row: softmax(q K^T * scale) V over the row's first ctx_len cached tokens, every head of
    the row in one batched product (GQA: G query heads per kv head).  Rows of one sequence share
    one gather of its K/V (the longest context among them)."""
    rows = q.shape[0]
    G = n_q_heads // n_kv_heads
    ctx = [int(c) for c in ctx_lens[:rows]]
    sids = [int(s) for s in seq_ids[:rows]]
    cache = {}
    for r in range(rows):
        n, seq = ctx[r], sids[r]
        if n == 0:
            out[r, : n_q_heads * head_dim] = 0
            continue
        if seq not in cache:
            nmax = max(c for c, s in zip(ctx, sids) if s == seq)
            cache[seq] = _gather_kv_heads(kv, seq, nmax, n_kv_heads)
        K, V = cache[seq]
        K, V = K[:, :n], V[:, :n]
        qv = q[r, : n_q_heads * head_dim].float().view(n_kv_heads, G, head_dim)
        p = torch.softmax(torch.einsum("hgd,hnd->hgn", qv, K) * scale, dim=-1)
        o = torch.einsum("hgn,hnd->hgd", p, V)
        out[r, : n_q_heads * head_dim] = o.reshape(-1).to(out.dtype)
    return out


def flash_attention(q, kv, *, Sk, n_kv_heads, causal, scale, q_offset=0, out, k_lens=None, q_offsets=None):
    B, Sq, Hq, D = q.shape
    G = Hq // n_kv_heads
    for b in range(B):
        sk = int(k_lens[b]) if k_lens is not None else Sk
        qo = int(q_offsets[b]) if q_offsets is not None else q_offset
        K, V = _gather_kv_heads(kv, b, sk, n_kv_heads)  # [Hkv, sk, D]
        qq = q[b].float().view(Sq, n_kv_heads, G, D)
        s = torch.einsum("qhgd,hkd->hgqk", qq, K) * scale
        if causal:
            qi = torch.arange(Sq)[:, None] + qo
            kj = torch.arange(sk)[None, :]
            s = s.masked_fill(kj > qi, float("-inf"))
        p = torch.softmax(s, dim=-1)
        o = torch.einsum("hgqk,hkd->qhgd", p, V)
        out[b] = o.reshape(Sq, Hq, D).to(out.dtype)
    return out


def _splitmix64(x: int) -> int:
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def gumbel_keys(logits_row: torch.Tensor, T: float, seed: int, step: int, row: int, v_offset: int = 0) -> torch.Tensor:
    """Exact replica of the kernel's counter-based Gumbel noise (vectorised); column j is global
    token id v_offset + j (a vocab shard under tensor parallelism)."""
    m = (1 << 64) - 1
    base = _splitmix64((seed & m) ^ _splitmix64((step * 0x100000001B3 + row) & m))
    V = logits_row.shape[0]
    v = torch.arange(v_offset, v_offset + V, dtype=torch.int64)
    # vectorised splitmix64 on uint64 emulated with python ints is slow; use numpy uint64
    import numpy as np

    x = (np.uint64(base) ^ v.numpy().astype(np.uint64))
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    u = ((x >> np.uint64(41)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)
    g = -np.log(-np.log(u))
    return logits_row.float() / T + torch.from_numpy(g.astype(np.float32))


def sample_partial(logits, *, mask, temperature, seed, step, v_offset=0):
    """Per-row best (key, global token id) over a logits shard whose column j is token
    v_offset + j: the kernel's partial stage (no step advance).  (-inf, -1) for an empty row."""
    rows, V = logits.shape
    sd = int(seed.reshape(-1)[0]) & ((1 << 64) - 1)
    st = int(step.reshape(-1)[0])
    vals = torch.full((rows,), float("-inf"), dtype=torch.float32)
    idx = torch.full((rows,), -1, dtype=torch.int64)
    lg = logits.detach().float().cpu()
    for r in range(rows):
        T = float(temperature[r]) if temperature is not None else 0.0
        key = gumbel_keys(lg[r], T, sd, st, r, v_offset) if T > 0 else lg[r].clone()
        if mask is not None:
            words = mask[r].detach().cpu().to(torch.int64) & 0xFFFFFFFF
            bits = ((words[:, None] >> torch.arange(32)[None, :]) & 1).reshape(-1)[v_offset : v_offset + V].bool()
            key = key.masked_fill(~bits, float("-inf"))
        if not (torch.isinf(key).all() and key.max() < 0):
            j = int(torch.argmax(key))  # first maximum: the lowest id wins ties, as in the kernel
            vals[r], idx[r] = key[j], v_offset + j
    return vals, idx


def merge_partials(vals: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """[n_src, rows] partial maxima -> token per row (largest key, lowest id on ties; -1 if none)."""
    n_src, rows = vals.shape
    out = torch.full((rows,), -1, dtype=torch.int64)
    for r in range(rows):
        best_v, best_i = float("-inf"), -1
        for p in range(n_src):
            v, i = float(vals[p, r]), int(idx[p, r])
            if i < 0:
                continue
            if best_i < 0 or v > best_v or (v == best_v and i < best_i):
                best_v, best_i = v, i
        out[r] = best_i
    return out


def sample(logits, *, mask, temperature, seed, step, out_tokens, v_offset=0):
    vals, idx = sample_partial(logits, mask=mask, temperature=temperature, seed=seed, step=step, v_offset=v_offset)
    out_tokens[: logits.shape[0]] = idx.to(out_tokens.dtype).to(out_tokens.device)
    step.add_(1)
    return out_tokens


def pcm16_to_f32(pcm, ratio, out):
    n_out = out.numel()
    if ratio == 1.0:
        out.copy_(pcm[:n_out].float() / 32768.0)
        return out
    src = torch.arange(n_out, dtype=torch.float64) * ratio
    j = src.floor().long()
    f = (src - j).float()
    j1 = (j + 1).clamp(max=pcm.numel() - 1)
    j = j.clamp(max=pcm.numel() - 1)
    out.copy_(((1 - f) * pcm[j].float() + f * pcm[j1].float()) / 32768.0)
    return out


def _g711_table(law: str) -> torch.Tensor:
    """code -> the standard's 16-bit value, int32 [256] (the arithmetic of csrc/ingest/ingest_resample.hip)."""
    c = torch.arange(256, dtype=torch.int32)
    if law == "mulaw":
        u = ~c & 0xFF
        t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)
        return torch.where((u & 0x80) != 0, 0x84 - t, t - 0x84)
    a = c ^ 0x55
    seg = (a >> 4) & 7
    t = (a & 0x0F) << 4
    t = torch.where(seg == 0, t + 8, (t + 0x108) << (seg - 1).clamp(min=0))
    return torch.where((a & 0x80) != 0, t, -t)


def ingest(raw, encoding, channels, channel, L, M, H, table, out):
    """csrc/ingest/ingest.h on host tensors, in its order of operations: decode, x (1 / 32768), the
    f32 mean in channel order (or the one channel), then per output the 2H taps in ascending order
    in f32 (a product and a sum per tap, each rounded; the kernel fuses the two).  raw: uint8, whole
    frames; out: f32 [>= n_in * L // M].  Returns out[:n_out]."""
    if encoding == "linear16":
        v = raw.view(torch.int16).to(torch.int32)
    else:
        v = _g711_table(encoding)[raw.long()]
    v = v.reshape(-1, channels).float() * (1.0 / 32768.0)
    n_in = v.shape[0]
    if channel is not None:
        x = v[:, channel]
    else:
        x = v[:, 0]
        for c in range(1, channels):
            x = x + v[:, c]
        if channels > 1:
            x = x / float(channels)
    n_out = n_in * L // M
    if L == M:
        out[:n_out].copy_(x)
        return out[:n_out]
    q = torch.arange(n_out, dtype=torch.int64) * M
    pos = torch.div(q, L, rounding_mode="floor")
    ph = q - pos * L
    xp = torch.cat([torch.zeros(H, dtype=torch.float32), x, torch.zeros(H + 1, dtype=torch.float32)])  # x[j] at j + H
    acc = torch.zeros(n_out, dtype=torch.float32)
    for k in range(2 * H):
        acc = acc + table[ph, k] * xp[pos + 1 + k]
    out[:n_out].copy_(acc)
    return out[:n_out]


def log_mel(audio, *, n_frames, window, mel_fb, out):
    """Whisper log-mel of a padded window -> out bf16 [n_frames, n_mels] (channels-last)."""
    stft = torch.stft(audio.float(), 400, 160, window=window.float(), center=True, pad_mode="reflect",
                      return_complex=True)
    mag = stft[..., :n_frames].abs() ** 2  # [201, frames]
    mel = mel_fb.float() @ mag
    lg = torch.clamp(mel, min=1e-10).log10()
    lg = torch.maximum(lg, lg.max() - 8.0)
    lg = (lg + 4.0) / 4.0
    out.copy_(lg.t().to(out.dtype))
    return out


def conv1d_gelu(x, w, b, *, stride, pos=None, out):
    B, Tin, Cin = x.shape
    Cout = w.shape[0]
    wt = w.float().view(Cout, 3, Cin).permute(0, 2, 1)  # [co, ci, kk]
    y = F.conv1d(x.float().transpose(1, 2), wt, None if b is None else b.float(), stride=stride, padding=1)
    y = F.gelu(y).transpose(1, 2)
    if pos is not None:
        y = y + pos[: y.shape[1]].float()[None]
    out.copy_(y.to(out.dtype))
    return out


def mel_filterbank(sr: int = 16000, n_fft: int = 400, n_mels: int = 80) -> torch.Tensor:
    """Slaney-style mel filterbank (librosa default, as used by Whisper) [n_mels, n_fft//2+1]."""

    def hz_to_mel(f):
        f = torch.as_tensor(f, dtype=torch.float64)
        f_sp = 200.0 / 3
        mels = f / f_sp
        min_log_hz = 1000.0
        min_log_mel = min_log_hz / f_sp
        logstep = math.log(6.4) / 27.0
        return torch.where(f >= min_log_hz, min_log_mel + torch.log(f / min_log_hz) / logstep, mels)

    def mel_to_hz(m):
        f_sp = 200.0 / 3
        freqs = f_sp * m
        min_log_hz = 1000.0
        min_log_mel = min_log_hz / f_sp
        logstep = math.log(6.4) / 27.0
        return torch.where(m >= min_log_mel, min_log_hz * torch.exp(logstep * (m - min_log_mel)), freqs)

    n_bins = n_fft // 2 + 1
    fftfreqs = torch.linspace(0, sr / 2, n_bins, dtype=torch.float64)
    mel_pts = torch.linspace(float(hz_to_mel(0.0)), float(hz_to_mel(sr / 2)), n_mels + 2, dtype=torch.float64)
    hz = mel_to_hz(mel_pts)
    fdiff = hz[1:] - hz[:-1]
    ramps = hz[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = torch.clamp(torch.minimum(lower, upper), min=0.0)
    enorm = 2.0 / (hz[2 : n_mels + 2] - hz[:n_mels])
    weights = weights * enorm[:, None]
    return weights.float()


# ----------------------------------------------------------------------------- word alignment
# (csrc/align: the same contracts in f32 torch / numpy)
def attn_probs(q, k, heads, n_keys, scale, out):
    """out[s, t, :n_keys] = softmax_j(scale * q[t, head s] . k[j, head s]); other columns untouched."""
    S, H, hd = k.shape
    qf = q.float().view(q.shape[0], H, hd)
    for s, h in enumerate(int(v) for v in heads.tolist()):
        sc = (qf[:, h] @ k[:n_keys, h].float().t()) * scale
        out[s, :, :n_keys] = torch.softmax(sc, dim=-1)
    return out


def align_cost(probs, n_tokens, n_keys, out):
    """out[:n_tokens, :n_keys] = -mean_h median7_j(z-score over the token rows); reflect padding,
    no filter when n_keys <= 3."""
    p = probs[:, :n_tokens, :n_keys].float()
    mu = p.mean(dim=1, keepdim=True)
    var = (p - mu).pow(2).mean(dim=1, keepdim=True)
    z = (p - mu) / torch.sqrt(var + 1e-12)
    if n_keys > 3:
        z = F.pad(z, (3, 3), mode="reflect").unfold(-1, 7, 1).sort(dim=-1).values[..., 3]
    out[:n_tokens, :n_keys] = -z.mean(dim=0)
    return out


def dtw_path(cost, n_tokens, n_keys, first_frame, last_frame):
    """f32 DTW (anti-diagonal order, as the kernel) with the tie rule diagonal < vertical <
    horizontal-by-default, and the backtrack from (n_tokens-1, n_keys-1)."""
    import numpy as np

    c = cost[:n_tokens, :n_keys].detach().cpu().numpy().astype(np.float32)
    T, N = c.shape
    inf = np.float32(np.inf)
    D = np.full((T + 1, N + 1), inf, dtype=np.float32)  # D[i+1][j+1]: cell (i, j)
    step = np.full((T, N), 2, dtype=np.int8)
    for d in range(T + N - 1):
        i = np.arange(max(0, d - N + 1), min(T, d + 1))
        j = d - i
        c0, c1, c2 = D[i, j], D[i, j + 1], D[i + 1, j]
        diag = (c0 < c1) & (c0 < c2)
        vert = ~diag & (c1 < c0) & (c1 < c2)
        best = np.where(diag, c0, np.where(vert, c1, c2))
        if d == 0:
            best = np.zeros(1, dtype=np.float32)
        D[i + 1, j + 1] = c[i, j] + best
        step[i, j] = np.where(diag, 0, np.where(vert, 1, 2))
    first = np.zeros(T, dtype=np.int64)
    last = np.zeros(T, dtype=np.int64)
    r, j = T - 1, N - 1
    last[r] = j
    while r > 0 or j > 0:
        s = 2 if r == 0 else 1 if j == 0 else int(step[r, j])
        if s != 2:
            first[r] = j
            r -= 1
            if s == 0:
                j -= 1
            last[r] = j
        else:
            j -= 1
    first_frame[:T] = torch.from_numpy(first).to(first_frame.dtype)
    last_frame[:T] = torch.from_numpy(last).to(last_frame.dtype)
    return first_frame, last_frame


def token_logprob(logits, targets, mask, vocab, out):
    """out[n] = logits[n, t_n] - logsumexp over allowed ids < vocab (mask: packed bits [N or 1, words])."""
    N = logits.shape[0]
    x = logits[:, :vocab].float()
    if mask is not None:
        ids = torch.arange(vocab)
        bits = (mask.reshape(-1, mask.shape[-1])[:, ids // 32] >> (ids % 32)) & 1
        x = x.masked_fill(bits.expand(N, -1) == 0, float("-inf"))
    t = targets[:N].long().clamp(0, vocab - 1)
    out[:N] = (x.gather(1, t[:, None])[:, 0] - torch.logsumexp(x, dim=-1)).clamp_max(0.0)
    return out


def sot_probe(logits, vocab, lang0, n_lang, allow, no_speech_id, lang_probs, lang_tok, lang_conf, no_speech,
              tok_dst=None, dst_rows=None):
    """Start-of-transcript probe (csrc/sot/sot.h): per row the softmax over ids < vocab at
    no_speech_id, the softmax over the allowed language ids (allow: int bit set, bit i = language
    lang0 + i; exactly 0 elsewhere), the lowest allowed id holding the raw maximum (an id of the set
    whatever the logits hold), its probability, and the token patch tok_dst[dst_rows[r]] = id."""
    R = logits.shape[0]
    x = logits[:, :vocab].float()
    no_speech[:R] = torch.softmax(x, dim=-1)[:, no_speech_id]
    on = torch.tensor([(allow >> i) & 1 == 1 for i in range(n_lang)])
    xl = x[:, lang0 : lang0 + n_lang].masked_fill(~on, float("-inf"))
    ml = torch.nan_to_num(xl, nan=float("-inf")).amax(dim=-1, keepdim=True)
    e = torch.exp(xl - ml)  # (every allowed logit -inf: NaN, as the kernel gives)
    p = torch.where(on, e / torch.where(on, e, torch.zeros(())).sum(-1, keepdim=True), torch.zeros(()))
    lang_probs[:R, :n_lang] = p
    idx = torch.arange(n_lang)
    hit = on & (xl == ml)
    best = torch.where(hit, idx, n_lang).amin(dim=-1)
    best = torch.where(best == n_lang, int(idx[on][0]), best)
    lang_tok[:R] = (lang0 + best).to(lang_tok.dtype)
    lang_conf[:R] = p.gather(1, best[:, None])[:, 0]
    if tok_dst is not None:
        for r in range(R):
            d = int(dst_rows[r])
            if 0 <= d < tok_dst.numel():
                tok_dst[d] = int(lang_tok[r])
    return lang_probs, lang_tok, lang_conf, no_speech


def beam_select(logits, cum, mask, vocab, W, cand_score, cand_beam, cand_tok):
    """Beam selection (csrc/beam/beam.h): rows are groups of W beams; a candidate (beam b, id v) of
    a group scores cum[row] + (x[v] - lse[row]) in f32, lse over the allowed ids < vocab; per group
    the 2 W best finite scores, descending, equal scores by ascending b * vocab + v, the tail
    (-inf, -1, -1)."""
    N = logits.shape[0]
    G, K = N // W, 2 * W
    x = logits[:, :vocab].float()
    if mask is not None:
        ids = torch.arange(vocab)
        bits = (mask.reshape(-1, mask.shape[-1])[:, ids // 32] >> (ids % 32)) & 1
        x = x.masked_fill(bits.expand(N, -1) == 0, float("-inf"))
    m = torch.nan_to_num(x, nan=float("-inf")).amax(dim=-1, keepdim=True)
    lse = m + torch.log(torch.exp(x - m).sum(dim=-1, keepdim=True))
    s = cum[:N].float()[:, None] + (x - lse)
    s = torch.where(torch.isfinite(s), s, torch.full((), float("-inf"))).reshape(G, W * vocab)
    # (a stable descending sort: equal scores keep the ascending flat index b * vocab + v)
    val, idx = torch.sort(s, dim=-1, descending=True, stable=True)
    val, idx = val[:, :K], idx[:, :K]
    if val.shape[1] < K:
        pad = K - val.shape[1]
        val = torch.cat([val, torch.full((G, pad), float("-inf"))], dim=1)
        idx = torch.cat([idx, torch.zeros(G, pad, dtype=idx.dtype)], dim=1)
    none = val == float("-inf")
    cand_score[:G, :K] = val
    cand_beam[:G, :K] = torch.where(none, -1, idx // vocab).to(cand_beam.dtype)
    cand_tok[:G, :K] = torch.where(none, -1, idx % vocab).to(cand_tok.dtype)
    return cand_score, cand_beam, cand_tok


def kv_beam_gather(k_cache, v_cache, block_table, slots, parents, n_ctx, max_ctx):
    """The beams' K/V follow their parents, in place (csrc/beam/beam.h): caches
    [L, n_blocks, H, bs, hd]; for beam w of group g with parent p != w, blocks j <
    ceil(min(n_ctx[g], max_ctx) / bs) of slot slots[g][w] take the old content of slot slots[g][p]'s."""
    bs = k_cache.shape[3]
    n_blocks = k_cache.shape[1]
    sessions, bps = block_table.shape
    G, W = slots.shape
    for cache in (k_cache, v_cache):
        for g in range(G):
            ctx = min(max(int(n_ctx[g]), 0), bps * bs, int(max_ctx))
            moves = []
            for w in range(W):
                p = int(parents[g, w])
                sd = int(slots[g, w])
                if p == w or not 0 <= p < W or not 0 <= sd < sessions:
                    continue
                ss = int(slots[g, p])
                if not 0 <= ss < sessions:
                    continue
                for j in range((ctx + bs - 1) // bs):
                    bd, bsrc = int(block_table[sd, j]), int(block_table[ss, j])
                    if 1 <= bd < n_blocks and 1 <= bsrc < n_blocks:
                        moves.append((bd, cache[:, bsrc].clone()))  # every source is read before any write
            for bd, src in moves:
                cache[:, bd] = src
    return k_cache, v_cache


def boost_step(logits, vocab, edge_off, edge_tok, edge_next, edge_bias, state_root, roots, state_in, state_out,
               tokens=None, parents=None, W=1):
    """The keyterm boosting step on host tensors, rule by rule as csrc/boost/boost.h states it (one
    f32 add per boosted id, so the result is bitwise what the kernel gives)."""
    S, E = state_root.numel(), edge_tok.numel()
    rows = roots.numel()
    off, tok, nxt, root_of = edge_off.tolist(), edge_tok.tolist(), edge_next.tolist(), state_root.tolist()
    old = state_in.tolist()  # (every source state is read before any is written)

    def lst(s):
        lo, hi = off[s], off[s + 1]
        return range(lo, hi) if 0 <= lo <= hi <= E else range(0)

    def find(s, v):
        for e in lst(s):
            if tok[e] == v:
                return e
        return -1

    for r in range(rows):
        root = int(roots[r])
        if root < 0 or root >= S or root_of[root] != root:
            state_out[r] = old[r]
            continue
        s = root
        src = r
        if parents is not None:
            p = int(parents[r])
            src = (r // W) * W + p if 0 <= p < W else -1
        if 0 <= src < rows:
            s = old[src]
            if s < 0 or s >= S or root_of[s] != root:
                s = root
        if tokens is not None:
            t = int(tokens[r])
            if t < 0:
                state_out[r] = s
                continue
            e = find(s, t)
            if e < 0 and s != root:
                e = find(root, t)
            n = nxt[e] if e >= 0 else root
            s = n if 0 <= n < S and root_of[n] == root else root
        state_out[r] = s
        mine = set()
        for e in lst(s):
            if 0 <= tok[e] < vocab:
                logits[r, tok[e]] += edge_bias[e]
            mine.add(tok[e])
        if s != root:
            for e in lst(root):
                if 0 <= tok[e] < vocab and tok[e] not in mine:
                    logits[r, tok[e]] += edge_bias[e]
    return logits, state_out


def ts_rules_step(logits, vocab, eot, ts_begin, max_initial, mask, enable, state_in, state_out, tokens=None):
    """The timestamp rules step on host tensors, rule by rule as csrc/tsrules/tsrules.h states it
    (T in f64: the kernel's f32 T decides differently only where T and M all but tie)."""
    rows = enable.numel()
    n_ts = vocab - ts_begin
    ninf = float("-inf")
    old = state_in[:rows].tolist()  # (in place: every row's cells are read before they are written)
    ids = torch.arange(vocab)
    for r in range(rows):
        t = None if tokens is None else int(tokens[r])
        if int(enable[r]) <= 0 or (t is not None and not 0 <= t < vocab):
            state_out[r] = torch.tensor(old[r], dtype=torch.int32)
            continue
        n, last, prev, last_ts = old[r]
        if not 0 <= n <= 2 or not -1 <= last_ts < n_ts:
            n, last, prev, last_ts = 0, -1, -1, -1
        if t is not None:
            prev, last, n = last, t, min(n + 1, 2)
            if t >= ts_begin:
                last_ts = t - ts_begin
        state_out[r] = torch.tensor([n, last, prev, last_ts], dtype=torch.int32)
        x = logits[r]
        m = mask[r if mask.shape[0] > 1 else 0]
        ok = ((m[ids >> 5] >> (ids & 31)) & 1).bool()  # allowed by the mask and not banned so far
        banned = torch.zeros(vocab, dtype=torch.bool)

        def ban(lo, hi):
            banned[max(lo, 0) : max(min(hi, vocab), 0)] = True

        ban(ts_begin - 1, ts_begin)
        last_was = n >= 1 and last >= ts_begin
        pen_was = n < 2 or prev >= ts_begin
        if last_was and pen_was:
            ban(ts_begin, vocab)
        elif last_was:
            ban(0, eot)
        if last_ts >= 0:
            ban(ts_begin, ts_begin + (last_ts if last_was and not pen_was else last_ts + 1))
        if n == 0:
            ban(0, ts_begin)
            if max_initial >= 0:
                ban(ts_begin + max_initial + 1, vocab)
        live = ok & ~banned
        xs = x[:vocab].double()
        ts, tx = xs[ts_begin:][live[ts_begin:]], xs[:ts_begin][live[:ts_begin]]
        T = float(torch.logsumexp(ts, 0)) if ts.numel() else ninf
        M = float(tx.max()) if tx.numel() else ninf
        if T > M:
            ban(0, ts_begin)
        x[:vocab][banned] = ninf
    return logits, state_out


def score_step(logits, vocab, eot, mask, enable, tokens, sum_in, sum_out, cnt_in, cnt_out, step_lp=None):
    """The score step on host tensors, as csrc/score/score.h states it (the log-sum-exp in f64,
    rounded to f32 once)."""
    rows = enable.numel()
    ninf = float("-inf")
    old_sum = sum_in[:rows].clone()  # (in place: every row's cells are read before they are written)
    old_cnt = cnt_in[:rows].clone()
    ids = torch.arange(vocab)
    for r in range(rows):
        t = int(tokens[r])
        n, done = int(old_cnt[r, 0]), int(old_cnt[r, 1])
        if int(enable[r]) <= 0 or done != 0 or not 0 <= t < vocab:
            sum_out[r] = old_sum[r]
            cnt_out[r] = old_cnt[r]
            if step_lp is not None:
                step_lp[r] = 0.0
            continue
        m = mask[r if mask.shape[0] > 1 else 0]
        ok = ((m[ids >> 5] >> (ids & 31)) & 1).bool()
        x = logits[r, :vocab].double()
        live = x[ok & (x > ninf)]
        lp = ninf
        if bool(ok[t]) and float(x[t]) > ninf and live.numel():
            lp = min(float(x[t] - torch.logsumexp(live, 0)), 0.0)
        lp32 = torch.tensor(lp, dtype=torch.float32)
        sum_out[r] = old_sum[r] + lp32
        cnt_out[r, 0] = n + 1
        cnt_out[r, 1] = int(t == eot)
        if step_lp is not None:
            step_lp[r] = lp32
    return sum_out, cnt_out


def set_logprob(logits, vocab, sets, out):
    """The set log-probability on host tensors, as csrc/turn/turn.h states it (both log-sum-exps in
    f64, rounded to f32 once)."""
    ninf = float("-inf")
    ids = torch.arange(vocab)
    for r in range(logits.shape[0]):
        s = sets[r if sets.shape[0] > 1 else 0]
        on = ((s[ids >> 5] >> (ids & 31)) & 1).bool()
        x = logits[r, :vocab].double()
        live = x > ninf  # (False for a NaN too)
        A = float(torch.logsumexp(x[live], 0)) if bool(live.any()) else ninf
        hit = live & on
        out[r, 0] = min(float(torch.logsumexp(x[hit], 0)) - A, 0.0) if bool(hit.any()) else ninf
        out[r, 1] = A
    return out


def seq_logprob(logits, vocab, target, end_set, seq, n_seq, acc_in, lp, acc_out):
    """The per-sequence log-probabilities on host tensors, as csrc/rescore/rescore.h states them: each
    row's value in f64, rounded to f32 once; the sums as f32 additions in row order."""
    ninf = float("-inf")
    ids = torch.arange(vocab)
    s = end_set.reshape(-1)
    on = ((s[ids >> 5] >> (ids & 31)) & 1).bool()
    for r in range(target.numel()):
        t = int(target[r])
        val = ninf
        if -1 <= t < vocab:
            x = logits[r, :vocab].double()
            live = x > ninf  # (False for a NaN too)
            if bool(live.any()):
                A = float(torch.logsumexp(x[live], 0))
                if t == -1:
                    hit = live & on
                    if bool(hit.any()):
                        val = min(float(torch.logsumexp(x[hit], 0)) - A, 0.0)
                elif bool(live[t]):
                    val = min(float(x[t]) - A, 0.0)
        lp[r] = val
    acc = torch.zeros(n_seq, dtype=torch.float32) if acc_in is None else acc_in.clone()
    for r in range(target.numel()):
        k = int(seq[r])
        if 0 <= k < n_seq:
            acc[k] = acc[k] + lp[r]  # f32 + f32, in row order
    acc_out.copy_(acc)
    return lp, acc_out


def _pack_bits32(on: torch.Tensor, words: int) -> torch.Tensor:
    """bool [n <= 32 words] -> the sampler's packed allow-bits, int32 [words]."""
    bits = torch.zeros(words * 32, dtype=torch.int64)
    bits[:on.numel()] = on.long()
    v = (bits.view(words, 32) << torch.arange(32)).sum(1)
    return torch.where(v >= 1 << 31, v - (1 << 32), v).to(torch.int32)


def nucleus_step(logits, vocab, mask_in, mask_out, n_kept, temperature, top_p, top_k, penalty, history):
    """The nucleus step on host tensors, as csrc/nucleus/nucleus.h states it, in f32: the penalty once
    per distinct valid id, (logit descending, id ascending) candidates, the cut of the renormalised
    top-k, pass-through rows.  The weights' sum runs left to right here (the kernel's order is its
    own): the two agree wherever no c_j / C lies within rounding of top_p."""
    ninf = float("-inf")
    words = (vocab + 31) // 32
    ids = torch.arange(vocab)
    for r in range(logits.shape[0]):
        x = logits[r]
        th = penalty[r]
        if float(th) != 1.0:
            seen = set()
            for t in history[r].tolist():
                if 0 <= t < vocab and t not in seen:
                    seen.add(t)
                    x[t] = x[t] / th if float(x[t]) > 0.0 else x[t] * th
        if mask_in is None:
            on = torch.ones(vocab, dtype=torch.bool)
        else:
            row = mask_in[r if mask_in.shape[0] > 1 else 0]
            on = ((row[ids >> 5] >> (ids & 31)) & 1).bool()
        T, p = float(temperature[r]), float(top_p[r])
        k = min(max(int(top_k[r]), 0), 1024)
        keep_all = not p < 1.0
        mask_out[r].zero_()
        if not T > 0.0 or (k == 0 and keep_all):
            mask_out[r, :words] = _pack_bits32(on, words)
            n_kept[r] = int(on.sum())
            continue
        if k == 0:
            k = 1024
        cand = ids[on & (x[:vocab] > ninf)]
        k = min(k, cand.numel())
        if k == 0:
            n_kept[r] = 0
            continue
        order = torch.sort(x[cand], descending=True, stable=True).indices[:k]   # ties keep id order
        K = cand[order]
        l = x[K]
        n = k
        if not keep_all:
            c = torch.cumsum(torch.exp((l - l[0]) / temperature[r]), 0)
            hit = torch.nonzero(c >= top_p[r] * c[-1])
            n = int(hit[0]) + 1 if hit.numel() else k
        keep = torch.zeros(vocab, dtype=torch.bool)
        keep[K[:n]] = True
        mask_out[r, :words] = _pack_bits32(keep, words)
        n_kept[r] = n
    return mask_out
