"""The rollout session (sea_amd/rollout_session.py) on the clock:

  (a) ms per single `step()` driven from a Python loop, beside what a closed loop costs without a session: `rollout(n_steps=1)` from an ever-longer context;
  (b) ms per step of `advance(steps)`, beside the same rollout through `rollout(mode='kv')`;
  (c) `fork(n)` from a history of k states — the whole call, and its sea_kv_cache_fork launch alone (device events around a batch of launches) with
      the bytes it moves and the GB/s it reaches —
      beside the other way to the same caches: the prefill (full-context forward + sea_kv_cache_fill) of the n-times-repeated history;
  (d) with --select: `fork(64)` from a history of k states, then `select` of 8 of the 64 members — the whole call, alternating with `open_rollout` on
      those 8 members' states and conditions (the only other way to such a session) — and the sea_kv_cache_gather launch alone over the same cache
      shapes in each of the four layout combinations (rows / V^T on either side), as bytes read + written per second, beside the rate of the
      fork(64) launch of the same run.  Only part (d) runs then; --out also writes what it prints to a file.

    python tools/session_bench.py [--widths cfg2,cylinder,multiphase] [--steps 100] [--k 1024] [--forks 8,64] [--dtype bf16]
    python tools/session_bench.py --select --out profiles/session_bench_select.txt

Widths as tools/context_rollout_bench.py: one layer, max_len 2024, B = 1.  Every figure is the median of --reps timed repeats after one warm-up
call.  Prints a table per part and one JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

WIDTHS = {"cfg2": (256, 3, "adaln"), "cylinder": (1024, 2, "adaln"), "multiphase": (2048, 2, "ln")}


def timed(fn, reps, setup=None):
    """Median wall time of fn() in ms (device drained before and after every repeat); setup() runs untimed before each."""
    out = []
    for i in range(reps + 1):
        if setup is not None:
            setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def timed_device(fn, reps, min_ms=20.0):
    """Median DEVICE time of one fn() in ms: every window is a batch of back-to-back launches between two events, sized so that it lasts at
    least `min_ms` (a single short launch inside a host-clocked, synchronised window would mostly measure the launch and the synchronise)."""
    fn()
    torch.cuda.synchronize()
    batch = 8
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        if e0.elapsed_time(e1) >= min_ms or batch >= 1 << 14:
            break
        batch *= 2
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / batch)
    return statistics.median(out)


SELECT_FORK = 64
SELECT_INDEX = (3, 9, 17, 22, 38, 41, 55, 60)


def select_leg(a, say):
    """Part (d) of the module docstring."""
    from sea_amd.models.temporal import TemporalModel
    from sea_amd.rollout_session import CacheFork, CacheGather
    from sea_amd.utils.train_utils import open_rollout

    k, index = a.k, list(SELECT_INDEX)
    dev = torch.device("cuda:0")
    esz = 2 if a.dtype == "bf16" else 4
    rows = []
    for wname in a.widths.split(","):
        E, F, ln = WIDTHS[wname]
        torch.manual_seed(42)
        model = TemporalModel(1, E, 8, 2024, 8, 0, F, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, ln)
        model.set_compute_dtype(a.dtype)
        model = model.to(dev).eval()
        eng = model.engine(dev)
        g = torch.Generator().manual_seed(77)
        x = torch.randn(1, k, F, E, generator=g).to(dev)
        ib = torch.rand(1, k, 1, generator=g).to(dev)
        src = open_rollout(model, x, ib[:, :k - 1].contiguous())
        wide = src.fork(SELECT_FORK)
        pos = wide.position
        row = dict(width=wname, E=E, F=F, ln=ln, k=k, fork=SELECT_FORK, index=index, forked_by=wide.forked_by, wide_fast=wide.fast)

        # select against open_rollout on the same 8 histories: alternating, each repeat drained before and after
        xs, cs = wide.states()[index].contiguous(), wide.conditions()[index].contiguous()
        made = []

        def drop():
            for t in made:
                t.close()
            made.clear()
        sel, opn = [], []
        for i in range(a.reps + 1):
            for out, fn in ((sel, lambda: wide.select(index)), (opn, lambda: open_rollout(model, xs, cs))):
                drop()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                made.append(fn())
                torch.cuda.synchronize()
                if i:
                    out.append((time.perf_counter() - t0) * 1e3)
        t = wide.select(index)
        row["selected_fast"], row["selected_by"] = t.fast, t.forked_by
        t.close()
        drop()
        row["select_ms"], row["open_rollout_ms"] = statistics.median(sel), statistics.median(opn)
        row["select_ms_all"], row["open_rollout_ms_all"] = sel, opn
        say(f"{wname:<11} fork({SELECT_FORK}) [{wide.forked_by}, {'value rows' if wide.fast else 'V^T'}] from k={k}, select of {len(index)} "
            f"[{'value rows' if row['selected_fast'] else 'V^T'}]: select() {row['select_ms']:.3f} ms   open_rollout on the same {len(index)} histories "
            f"{row['open_rollout_ms']:.3f} ms   ({'select is faster' if row['select_ms'] < row['open_rollout_ms'] else 'select is NOT faster'})")

        # the fork launch of this run
        if wide.forked_by == "copy":
            entries = [dict(src=p, dst=q, n_pos=pos, transposed=tr) for (p, tr), (q, _) in zip(src._caches(), wide._caches())]
            cf = CacheFork(entries, eng.act_dtype, "bench")
            elems = sum(p.shape[0] * p.shape[1] * (p.shape[2] if tr else p.shape[3]) * pos for p, tr in src._caches())
            ms = timed_device(cf.run, max(a.reps, 10))
            row["fork_launch"] = dict(ms=ms, bytes=elems * esz * (1 + SELECT_FORK), gbps=elems * esz * (1 + SELECT_FORK) / ms / 1e6)
            say(f"{wname:<11}   fork({SELECT_FORK}) launch           {ms:.4f} ms, {row['fork_launch']['bytes'] / 1e6:.1f} MB read + written, {row['fork_launch']['gbps']:.0f} GB/s")

        # the gather launch alone: every cache tensor of the 64-member session, 8 rows of it into an 8-row destination, in each layout combination
        shapes = [(c.shape[1], c.shape[2] if tr else c.shape[3], c.shape[3] if tr else c.shape[2]) for c, tr in wide._caches()]     # (H, hd, cap)
        src.close()
        wide.close()
        torch.cuda.empty_cache()
        dev_index = torch.tensor(index, dtype=torch.int32, device=dev)
        lay = lambda b, H, hd, cap, tr: (b, H, hd, cap) if tr else (b, H, cap, hd)
        row["gather_launch"] = {}
        for st, dt in ((0, 0), (1, 1), (0, 1), (1, 0)):
            srcs = [torch.zeros(lay(SELECT_FORK, H, hd, cap, st), device=dev, dtype=eng.act_dtype) for H, hd, cap in shapes]
            dsts = [torch.zeros(lay(len(index), H, hd, cap, dt), device=dev, dtype=eng.act_dtype) for H, hd, cap in shapes]
            cg = CacheGather([dict(src=p, dst=q, n_pos=pos, src_transposed=bool(st), dst_transposed=bool(dt)) for p, q in zip(srcs, dsts)], dev_index,
                             eng.act_dtype, "bench")
            nbytes = 2 * sum(len(index) * H * hd * pos for H, hd, _ in shapes) * esz
            ms = timed_device(cg.run, max(a.reps, 10))
            name = f"{'V^T' if st else 'rows'} -> {'V^T' if dt else 'rows'}"
            row["gather_launch"][name] = dict(ms=ms, bytes=nbytes, gbps=nbytes / ms / 1e6)
            say(f"{wname:<11}   gather launch {name:<12} {ms:.4f} ms, {nbytes / 1e6:.1f} MB read + written, {nbytes / ms / 1e6:.0f} GB/s")
            del srcs, dsts, cg
            torch.cuda.empty_cache()
        rows.append(row)
        del model, eng
        torch.cuda.empty_cache()
    say(json.dumps({"session_bench_select": rows, "dtype": a.dtype}))


def main():
    from sea_amd import kv_engine
    from sea_amd.models.temporal import TemporalModel
    from sea_amd.rollout_session import CacheFork
    from sea_amd.utils.train_utils import open_rollout, rollout

    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="cfg2,cylinder,multiphase")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--k", type=int, default=1024, help="history length of the fork part")
    ap.add_argument("--forks", default="8,64")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-steps", type=int, default=20, help="steps of the session-less closed loop (every one prefills its whole context)")
    ap.add_argument("--select", action="store_true", help="run part (d), the select leg, instead of parts (a) - (c)")
    ap.add_argument("--out", default=None, help="with --select: also write the output to this file")
    a = ap.parse_args()
    if a.select:
        lines = []

        def say(text):
            print(text, flush=True)
            lines.append(text)
        select_leg(a, say)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    n, k, forks = a.steps, a.k, [int(v) for v in a.forks.split(",")]
    dev = torch.device("cuda:0")
    esz = 2 if a.dtype == "bf16" else 4
    rows = []
    for wname in a.widths.split(","):
        E, F, ln = WIDTHS[wname]
        torch.manual_seed(42)
        model = TemporalModel(1, E, 8, 2024, 8, 0, F, 2, 0.0, "sea", "learnable", "mlp", "add", 1, 1, True, ln)
        model.set_compute_dtype(a.dtype)
        model = model.to(dev).eval()
        eng = model.engine(dev)
        g = torch.Generator().manual_seed(77)
        x = torch.randn(1, k, F, E, generator=g).to(dev)
        ib = torch.rand(1, k + n + a.loop_steps, 1, generator=g).to(dev)
        row = dict(width=wname, E=E, F=F, ln=ln, steps=n, k=k, fast=kv_engine.supported(eng, 1))

        # (a) single steps from a Python loop; (b) advance against rollout(mode='kv'): both from one known state
        s = open_rollout(model, x[:, :1].contiguous(), ib[:, :0])
        s.step(ib[:, 0])

        def step_loop():
            for i in range(n):
                s.step(ib[:, i])
        row["step_ms"] = timed(step_loop, a.reps, setup=lambda: s.rewind(0)) / n
        fut = ib[:, :n].contiguous()
        row["advance_ms_per_step"] = timed(lambda: s.advance(fut), a.reps, setup=lambda: s.rewind(0)) / n
        x1 = x[:, :1].contiguous()
        row["rollout_kv_ms_per_step"] = timed(lambda: rollout(model, x1, ib, n, mode="kv"), a.reps) / n
        s.close()

        def bare_loop():   # a closed loop without a session: every step prefills the context it has grown so far
            ctx = x[:, :64].contiguous()
            for i in range(a.loop_steps):
                ctx = torch.cat((ctx, rollout(model, ctx, ib, 1, mode="kv")), dim=1)
        row["no_session_ms_per_step_from_k64"] = timed(bare_loop, 2) / a.loop_steps
        print(f"{wname:<11} step() {row['step_ms']:.4f} ms   advance {row['advance_ms_per_step']:.4f} ms/step   rollout(kv) {row['rollout_kv_ms_per_step']:.4f} ms/step"
              f"   session-less closed loop from k=64 {row['no_session_ms_per_step_from_k64']:.3f} ms/step", flush=True)

        # (c) fork against the prefill of the repeated history
        src = open_rollout(model, x, ib[:, :k - 1].contiguous())
        for nf in forks:
            made = []
            fork_ms = timed(lambda: made.append(src.fork(nf)), a.reps, setup=lambda: [t.close() for t in made] and made.clear())
            t = made[-1]
            f = dict(n=nf, forked_by=t.forked_by, fork_ms=fork_ms)
            if t.forked_by == "copy":
                entries = [dict(src=p, dst=q, n_pos=src.position, transposed=tr) for (p, tr), (q, _) in zip(src._caches(), t._caches())]
                cf = CacheFork(entries, eng.act_dtype, "bench")
                elems = sum(p.shape[0] * p.shape[1] * (p.shape[2] if tr else p.shape[3]) * src.position for p, tr in src._caches())
                f["copy_ms"] = timed_device(cf.run, max(a.reps, 10))
                f["bytes_read"], f["bytes_written"] = elems * esz, elems * esz * nf
                f["gbps"] = (f["bytes_read"] + f["bytes_written"]) / f["copy_ms"] / 1e6
            xr, ir = src.states().repeat_interleave(nf, dim=0), src.conditions().repeat_interleave(nf, dim=0)
            opened = []
            f["prefill_open_ms"] = timed(lambda: opened.append(eng.open_rollout(xr, ir)), 3, setup=lambda: [o.close() for o in opened] and opened.clear())
            with torch.no_grad():
                f["prefill_forward_ms"] = timed(lambda: eng.forward(xr[:, :k - 1].contiguous(), ir), 3)
            for o in opened + made:
                o.close()
            row[f"fork{nf}"] = f
            print(f"{wname:<11} fork({nf}) from k={k}: {f['forked_by']:<8} fork() {fork_ms:.3f} ms" +
                  (f"   launch {f['copy_ms']:.4f} ms, {(f['bytes_read'] + f['bytes_written']) / 1e6:.1f} MB, {f['gbps']:.0f} GB/s" if "copy_ms" in f else "") +
                  f"   prefill of the repeated history: open {f['prefill_open_ms']:.3f} ms (forward alone {f['prefill_forward_ms']:.3f} ms)", flush=True)
            del xr, ir
            torch.cuda.empty_cache()
        src.close()
        rows.append(row)
        del model, eng
        torch.cuda.empty_cache()
    print(json.dumps({"session_bench": rows, "dtype": a.dtype}))


if __name__ == "__main__":
    main()
