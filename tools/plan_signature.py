"""Launch-list signatures of sea_amd plans, built in HOST memory (no GPU): run at two commits from the repository root and diff the two outputs.
Per record: name, C function, lane, scalar arguments and a hash over every field of every argument struct, each pointer replaced by "(buffer kind, shape,
dtype) + byte offset" — allocation order may differ between the two commits, what a launch reads and writes may not.  Uses only API that a plan change
is unlikely to touch (TemporalEngine.plan, Plan(...), kv_engine.cond_plan_for, TrainPlan(...), records, _all_records(), _keep).
usage: python tools/plan_signature.py [--jobs N] > out.json        (needs libsea_hip.so built: python -m sea_amd.build)"""
import os, sys, json, hashlib, inspect, textwrap, ctypes as C
from concurrent.futures import ProcessPoolExecutor
sys.path.insert(0, os.getcwd())
import torch
from sea_amd import engine as Eg, _native as N, ptrcheck
from oracle import sea_oracle as O

N.lib()
Eg.FlatParams.sync = lambda self, force=False: None              # the two device launches of a plan's construction
Eg.FlatParams.sync_transposed = lambda self, force=False: None
if hasattr(Eg, "_require_gpu"):                                   # the device guard: its seam, or (commits before the seam) the constructor without it
    Eg._require_gpu = lambda device: None
    _init = Eg.TemporalEngine.__init__
else:
    _ns = {}
    exec(textwrap.dedent(inspect.getsource(Eg.TemporalEngine.__init__).replace('if device.type != "cuda":', 'if False:')), Eg.__dict__, _ns)
    _init = _ns["__init__"]


def make(cfg, dt):
    from sea_amd.models.temporal import TemporalModel
    m = TemporalModel(cfg.num_layers, cfg.embed_dim, cfg.n_heads, cfg.max_len, cfg.scale_ratio, cfg.src_len, cfg.num_variables, cfg.down_proj, 0.0,
                      cfg.exchange_mode, "learnable", cfg.ib_scale_mode, cfg.ib_addition_mode, 1, 1, cfg.add_info_after_cross, cfg.LN_type)
    e = Eg.TemporalEngine.__new__(Eg.TemporalEngine)
    _init(e, m, torch.device("cpu"), dt)
    return e


def ranges(plan, extra=()):
    eng, out = plan.eng, []
    def add(t, label):
        if isinstance(t, torch.Tensor) and t.numel():
            st = t.untyped_storage()
            out.append((st.data_ptr(), st.data_ptr() + st.nbytes(), label))
    def walk(o, label):
        if isinstance(o, torch.Tensor):
            add(o, f"{label}{tuple(o.shape)}{str(o.dtype)[6:]}")
        elif isinstance(o, (list, tuple)):
            for x in o:
                walk(x, label)
        elif hasattr(o, "_keep") and o is not plan:
            walk(o._keep, "cond")
    walk(plan._keep, "ws")
    P = eng.params
    for t, l in ((P.flat32, "flat32"), (P.flat_act, "flat_act"), (P.flat_actT, "flat_actT"), (eng.grads, "grads"), (eng.rope_self, "rope_s"), (eng.rope_cross, "rope_c"),
                 (getattr(plan, "_ws_colsum", None), "colsum")):
        add(t, l)
    for k, t in eng._eyes.items():
        add(t, f"eye{k}")
    for t in extra:
        add(t, "x")
    return out


def norm_ptr(p, R):
    for lo, hi, label in R:
        if lo <= p < hi:
            return f"{label}+{p - lo}"
    return "?"   # a host pointer (struct of the same record) or an unbound caller pointer


def sig(plan):
    R = ranges(plan)
    recs = plan._all_records()
    out = []
    for r in recs:
        fn = getattr(r.fn, "__name__", None)
        items = []
        roots = [a for a in r.args if isinstance(a, (C.Structure, C.Array))] + ([r.keep] if r.keep is not None else [])
        seen = set()
        for root in roots:
            for st in ptrcheck._walk_structs(root):
                if C.addressof(st) in seen:
                    continue
                seen.add(C.addressof(st))
                for name, typ in st._fields_:
                    v = getattr(st, name)
                    if typ is C.c_void_p:
                        items.append((type(st).__name__, name, norm_ptr(v, R) if v else None))
                    elif isinstance(v, (int, float)):
                        items.append((type(st).__name__, name, v))
                    elif isinstance(v, C.Array) and getattr(v, "_type_", None) is C.c_void_p:
                        items.append((type(st).__name__, name, [norm_ptr(x, R) if x else None for x in v]))
        scal = [(norm_ptr(a, R) if isinstance(a, int) and a >= 1 << 32 else a) for a in r.args if isinstance(a, (int, float)) or a is None]
        out.append([r.name, fn, r.lane, scal, hashlib.sha1(repr(items).encode()).hexdigest()[:12]])
    patches = sorted((len(getattr(plan, k, ())) for k in ("_x_patches", "_out_patches", "_c_patches", "_pos_structs", "_drop_structs", "_hoisted", "_dout_patches")))
    return dict(records=out, patches=patches, native_list=plan._clist is not None)


def cases():
    C_ = O.OracleConfig
    models = {
        "cfg2": C_(1, 256, 8, 2048, 8, 0, 3, 2, True, "adaln"),
        "cfg2_ln": C_(1, 256, 8, 2048, 8, 0, 3, 2, True, "ln"),
        "cfg2_pre": C_(1, 256, 8, 2048, 8, 0, 3, 2, False, "adaln"),
        "cfg2_L2": C_(2, 256, 8, 2048, 8, 0, 3, 2, True, "adaln"),
        "cfg2_F2": C_(1, 256, 8, 2048, 8, 0, 2, 2, True, "adaln"),
        "cfg2_F1": C_(1, 256, 8, 2048, 8, 0, 1, 2, True, "adaln"),
        "e128": C_(1, 128, 8, 256, 8, 0, 3, 2, True, "adaln"),
        "cyl": C_(1, 1024, 8, 400, 8, 0, 2, 2, True, "adaln"),
        "mph": C_(1, 2048, 8, 200, 8, 0, 2, 2, True, "ln"),
        "hd48": C_(1, 384, 8, 128, 8, 0, 3, 2, True, "adaln"),
    }
    for xm, ibm, ibs, after in (("addition", "add", "mlp", True), ("simple", "add", "mlp", True), ("pool", "add", "mlp", True), ("sea", "none", "mlp", True),
                                ("sea", "attention", "mlp", True), ("sea", "attention", "mlp", False), ("sea", "concat", "mlp", False), ("sea", "add", "fourier", True), ("sea", "add", "linear", False)):
        models[f"v_{xm}_{ibm}_{ibs}_{int(after)}"] = C_(1, 64, 4, 128, 8, 0, 3, 2, after, "adaln", xm, ibm, ibs)
        models[f"w_{xm}_{ibm}_{ibs}_{int(after)}"] = C_(1, 256, 8, 512, 8, 0, 3, 2, after, "adaln", xm, ibm, ibs)
    return models


SWITCHES = ["", "lanes=all", "lanes=cond", "lanes=none", "norm=0", "xtail=0", "chain=0", "riders=0", "silu=1", "silu=0", "fold_ib=0", "fold_ib_gen=1", "mlp1=1", "mlp1=0", "mlp1=1,mlp2=1",
            "mlp1=1,mlp2=1,mlpblock=0", "mlp2=0", "mlpnorm=0", "mlpnorm=1", "mlpblock=0", "front=0", "front3=0", "front_big=1", "adaln_gemm=0", "projnorm=0", "splitk=0", "rider_caps=256:64:64",
            "chain_max_rows=1000", "xtail_max_rows=100"]

def run_model(job):
    """Every plan of one (model, dtype): {key: signature | error text}, number of unexpected errors."""
    from sea_amd import kv_engine
    from sea_amd.train_engine import TrainPlan
    mname, dt = job
    torch.set_num_threads(1)
    cfg = cases()[mname]
    res, bad = {}, 0
    for sw in (SWITCHES if mname in ("cfg2", "cfg2_pre", "cfg2_ln", "cyl") else [""]):
        os.environ["SEA_PLAN"] = sw
        T = min(cfg.max_len, 2024)
        shapes = [(1, T, "full"), (8, T, "full"), (1, 70, "full"), (16, 70, "full"), (1, 1, "step"), (4, 1, "step")]
        for kvsw in ("", "gemv=0"):
            os.environ["SEA_KV"] = kvsw
            for (B, T_, mode) in shapes:
                if kvsw and mode != "step":
                    continue
                key = f"{mname}|{str(dt)[6:]}|{sw}|{kvsw}|{B}x{T_}|{mode}"
                try:
                    e = make(cfg, dt)
                    p = e.plan(B, T_, mode)
                    res[key] = sig(p)
                    if mode == "step" and sw == "" and cfg.ib_addition_mode in ("add", "none"):
                        cp = kv_engine.cond_plan_for(e, 5 * B)
                        res[key + "|cond"] = sig(cp)
                        res[key + "|hoisted"] = sig(Eg.Plan(e, B, 1, "step", cond=cp))
                    if mode == "full" and sw in ("", "splitk=0") and B * T_ <= 4096:
                        for thr, dx in ((0, False), (26, True)):
                            tp = TrainPlan(e, B, T_, drop_thr=thr, dp=False, want_dx=dx, want_dc=dx)
                            res[key + f"|train{thr}{int(dx)}"] = sig(tp)
                except NotImplementedError:
                    res[key] = "NotImplementedError"
                except Exception as ex:
                    bad += 1
                    res[key] = f"{type(ex).__name__}: {ex}"[:200]
    return res, bad


if __name__ == "__main__":
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else min(8, os.cpu_count() or 1)
    work = [(mname, dt) for mname in cases() for dt in (torch.bfloat16, torch.float32)]
    work.sort(key=lambda j: j[0] not in ("cfg2", "cfg2_pre", "cfg2_ln", "cyl"))   # the models with the switch matrix first
    res, bad = {}, 0
    with ProcessPoolExecutor(jobs) as pool:
        for r, b in pool.map(run_model, work):
            res.update(r)
            bad += b
    json.dump(res, sys.stdout, indent=0, sort_keys=True)
    print(f"{len(res)} plans, {bad} errors", file=sys.stderr)
