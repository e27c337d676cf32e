"""Timing probe of the fused optimizer update (rho_optim_step) and the gradient-norm reduction, quoted in DESIGN.md section 7
"Optimizers".  Not a product path.

    python tools/optim_probe.py [--n 166800000] [--out DIR]            (DIR: $RHO_RUN_OUT, else runs/)

Scratch arenas of --n float32 (default: the c3 model's arena, 166.8 M).  HIP events around each launch, median of --iters launches
after --warmup calls, per optimizer kind (the option set with the most state traffic and the plain one where they differ), time and
TB/s over the kind's algorithmic bytes: p read + written, g read, each state arena read + written (SGD's first step only writes its
buffer; the probe times step 2).  Then the two launches of the norm reduction, and rho_adamw against the AdamW kind of the new
kernel, alternated launch by launch in this one process.  Prints one JSON line and writes it to DIR/optim_probe.json."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# kind, label, flags, hp after (lr, weight_decay, eps), state arenas used, bytes per element
ROWS = [
    ("AdamW", "AdamW", 0, (0.9, 0.999), 2, 28),
    ("AdamW", "AdamW amsgrad", 2, (0.9, 0.999), 3, 36),
    ("Adam", "Adam", 0, (0.9, 0.999), 2, 28),
    ("SGD", "SGD", 0, (0.0, 0.0), 0, 12),
    ("SGD", "SGD momentum nesterov", 8, (0.9, 0.0), 1, 20),
    ("RMSprop", "RMSprop", 0, (0.99, 0.0), 1, 20),
    ("RMSprop", "RMSprop centered momentum", 16, (0.99, 0.9), 3, 36),
    ("Adagrad", "Adagrad", 0, (0.0,), 1, 20),
    ("Adamax", "Adamax", 0, (0.9, 0.999), 2, 28),
    ("NAdam", "NAdam", 0, (0.9, 0.999, 4e-3, 0.2), 2, 28),
    ("RAdam", "RAdam rectified", 0, (0.9, 0.999), 2, 28),
    ("Adadelta", "Adadelta", 0, (0.9,), 2, 28),
]


def timed(fns, iters: int, warmup: int):
    """Median device time in microseconds of each fn, the fns alternated launch by launch (one event pair per launch)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    pairs = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            pairs[k].append((a, b))
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) * 1e3 for a, b in p) for p in pairs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=166_800_000)
    ap.add_argument("--out", default=os.environ.get("RHO_RUN_OUT", "runs"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from rho_diffusion_amd.engine import ops
    n, dev = args.n, "cuda"
    p = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev) * 1e-2
    s = [torch.zeros(n, device=dev) for _ in range(3)]
    step = 1000                                                 # RAdam: rectified; SGD: past the seeding step
    rows = []
    for kind, label, flags, extra, n_state, bpe in ROWS:
        states = s[:n_state] if kind != "RMSprop" else [s[0], s[1] if flags & 16 else None, s[2] if extra[1] > 0 else None]
        for t in s:
            t.fill_(0.5 if kind == "Adagrad" else 0.0)
        fn = lambda: ops.optim_step(kind, p, g, states, (1e-4, 1e-2, 1e-8, *extra), step, flags)          # noqa: E731
        (us,) = timed([fn], args.iters, args.warmup)
        rows.append({"kind": label, "bytes_per_elem": bpe, "us": round(us, 1), "TBps": round(bpe * n / us * 1e-6, 2)})
    blocks = ops.sumsq_blocks(n)
    partials, out = torch.empty(blocks, device=dev), torch.empty(2, device=dev)
    us_part, us_fin = timed([lambda: ops.sumsq_partial(g, partials), lambda: ops.clip_coef(partials, 1.0, out)], args.iters, args.warmup)
    for t in s:
        t.zero_()
    us_old, us_new = timed([lambda: ops.adamw(p, g, s[0], s[1], 1e-4, 0.9, 0.999, 1e-8, 1e-2, step),
                            lambda: ops.optim_step("AdamW", p, g, s[:2], (1e-4, 1e-2, 1e-8, 0.9, 0.999), step)], args.iters, args.warmup)
    res = {"n": n, "iters": args.iters, "kinds": rows,
           "sumsq_partial": {"us": round(us_part, 1), "TBps": round(4 * n / us_part * 1e-6, 2), "blocks": blocks},
           "clip_coef": {"us": round(us_fin, 1)},
           "adamw_alternated": {"rho_adamw_us": round(us_old, 1), "rho_adamw_TBps": round(28 * n / us_old * 1e-6, 2),
                                "optim_step_adamw_us": round(us_new, 1), "optim_step_adamw_TBps": round(28 * n / us_new * 1e-6, 2)}}
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "optim_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
