"""Which inputs of tests/test_gpu_training_regimes.py and of tests/test_gpu_handle_reuse.py (its table: tests/handle_reuse_inputs.py) are
fit for tight bounds: orc.model_vjp in float32 against float64 on the CPU.

A pre-activation within fp32 rounding of a ReLU kink lands on the other side in float32, and the derivative through that unit differs
by percents in the rows behind it -- with no bug anywhere.  For every input of the two test modules (its graph, cfg, parameters and data,
imported from them) and both cotangents they use (step!'s loss; ybar of mgn_forward_vjp where the module runs it) this prints the worst
per-tensor error, the worst row of nfbar, the rows over 2e-5 and the whole-gradient relative L2, and exits non-zero if an input shows
a tensor over 1e-5 or a row over 2e-5: such an input must get another seed before a test relies on it.  One float32 run samples one
rounding pattern, and a kernel that sums in another order rounds differently, so a fit input must also hold still in float64 when
every parameter is moved by one fp32 rounding (ps (1 + 2^-24 n), n normal; 8 draws): the same two limits against the unperturbed
float64 result ("perturbed" below).  Under ln_dims = ALL float32 takes the whole-array statistics (4e5 to 1.2e6 values) in float32 and
is off by 1e-5 to 5e-5 in the LayerNorm parameters on every seed with no unit flipped, so there the float32 tensor limit is 1e-4 and the
perturbation test carries the kink criterion.  No GPU needed.

    python tools/train_regime_inputs.py [--search] [--reuse | --regimes]
        --search: for an unfit input, try the next seed bumps and name the first fit one
        --reuse / --regimes: only the inputs of test_gpu_handle_reuse.py / of test_gpu_training_regimes.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import mgn_oracle as orc
import test_gpu_training_regimes as T
import handle_reuse_inputs as H

TENSOR_MAX, ROW_MAX = 1e-5, 2e-5
bad = 0
# either module: INPUTS, inputs(name), SEED_BUMP, VJP_INPUTS and the cache _inputs
modules = [M for M, flag in ((T, "--reuse"), (H, "--regimes")) if flag not in sys.argv]
todo = [(M, name, None) for M in modules for name in M.INPUTS]
while todo:
    M, name, bump = todo.pop(0)
    if bump is not None:
        M.SEED_BUMP[name] = bump
        M._inputs.pop(name, None)
    d = M.inputs(name)
    fit = True
    for vjp in ((False, True) if name in M.VJP_INPUTS else (False,)):
        res = {}
        t0 = time.time()
        for dtype in (np.float64, np.float32):
            orc.LN_DIMS = "all" if d["lnall"] else "row"
            seed = (lambda out, dt=dtype: d["ybar"].astype(dt)) if vjp else T.loss_seed(d, dtype)
            _, gs, g_nf = orc.model_vjp(d["ps"], d["cfg"], d["nf"], d["ef"], d["s"], d["r"], seed, dtype=dtype, set2=d["set2"])
            orc.LN_DIMS = "row"
            res[dtype] = (np.asarray(gs, np.float64), np.asarray(g_nf, np.float64))
        (g64, n64), (g32, n32) = res[np.float64], res[np.float32]
        errs = T.tensor_errors(g32, g64, d["cfg"])
        worst = max(errs, key=errs.get)
        rows = T.nf_row_errors(n32, n64)
        l2 = np.linalg.norm(g32 - g64) / np.linalg.norm(g64)
        ok = errs[worst] <= (1e-4 if d["lnall"] else TENSOR_MAX) and rows.max() <= ROW_MAX
        pt = pr = 0.0
        # one fp32 rounding on every parameter, in float64; a module may ask for more (PERTURB_BITS, per input PERTURB_BITS_OF: 8 draws per entry)
        for bits in (getattr(M, "PERTURB_BITS_OF", {}).get(name, getattr(M, "PERTURB_BITS", (24,))) if ok else ()):
            prng = np.random.default_rng(5)
            for trial in range(8):
                ps = d["ps"].astype(np.float64) * (1.0 + 2.0 ** -bits * prng.standard_normal(d["ps"].size))
                orc.LN_DIMS = "all" if d["lnall"] else "row"
                seed = (lambda out: d["ybar"].astype(np.float64)) if vjp else T.loss_seed(d)
                _, gp, np_ = orc.model_vjp(ps, d["cfg"], d["nf"], d["ef"], d["s"], d["r"], seed, set2=d["set2"])
                orc.LN_DIMS = "row"
                pt = max(pt, max(T.tensor_errors(gp, g64, d["cfg"]).values()))
                pr = max(pr, float(T.nf_row_errors(np_, n64).max()))
            ok = pt <= TENSOR_MAX and pr <= ROW_MAX
        fit = fit and ok
        print(f"{name:24s} bump {M.SEED_BUMP.get(name, 0)}  {'ybar' if vjp else 'loss'}  N {d['N']:5d} E {d['E']:5d}  worst tensor {errs[worst]:.1e} ({worst})  worst nfbar row {rows.max():.1e}  "
              f"rows over {ROW_MAX}: {(rows > ROW_MAX).sum()}  gradient L2 {l2:.1e}  perturbed: tensor {pt:.1e} row {pr:.1e}  {'ok' if ok else 'UNFIT'}  ({time.time() - t0:.1f} s)", flush=True)
    if not fit and "--search" in sys.argv and M.SEED_BUMP.get(name, 0) < 40:
        todo.insert(0, (M, name, M.SEED_BUMP.get(name, 0) + 1))
    elif not fit:
        bad += 1
    elif bump is not None:
        print(f"    -> {M.__name__}.SEED_BUMP[{name!r}] = {bump}")
sys.exit(1 if bad else 0)
