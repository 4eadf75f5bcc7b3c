"""The dense Llama-3 LM head (128256 x 4096 bf16 = 1.05 GB, four times the Infinity Cache: nothing
of it survives from one launch to the next) through the streaming GEMM with the default and the
non-temporal weight policy (TiledWeight.nt -> SkinnyParams::w_nt), alternating in one process.

    python tools/wnt_lmhead.py [--rows 1] [--wnt 0,1,0,1] [--iters 40] [--json out.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice_enabled_browser_automation_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--wnt", default="0,1,0,1")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ops.ext()
    torch.manual_seed(0)
    w = ops.TiledWeight((torch.randn(a.vocab, a.hidden, device="cuda") * 0.02).to(torch.bfloat16))
    x = torch.randn(a.rows, a.hidden, device="cuda").to(torch.bfloat16)
    out = torch.empty(a.rows, a.vocab, dtype=torch.float32, device="cuda")
    ref = None
    for nt in [bool(int(v)) for v in a.wnt.split(",")]:
        w.nt = nt
        ts = []
        for i in range(a.iters + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.linear(x, w, out=out, fuse_rms=True, eps=1e-5)
            e1.record()
            e1.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1) * 1e3)
        if ref is None:
            ref = out.clone()
        med = statistics.median(ts)
        r = dict(tool="wnt_lmhead", rows=a.rows, vocab=a.vocab, hidden=a.hidden, wnt=nt, us=round(med, 2),
                 us_min=round(min(ts), 2), tb_s=round(w.numel() * 2 / (med * 1e-6) / 1e12, 3),
                 same_bits=bool(torch.equal(out, ref)))
        print(json.dumps(r), flush=True)
        if a.json:
            with open(a.json, "a") as f:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
