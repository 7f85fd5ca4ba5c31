"""Optimisers.Adam in float32, one rounding per operation: the arithmetic mgn_adam_update promises (include/mgn_hip.h), restated in NumPy
for tests/test_params_dev_host.py and tests/test_gpu_params_dev.py.  Every array and every scalar below is np.float32, so each NumPy
operation is one correctly rounded fp32 operation and nothing is fused; only beta_t lives in double, as in the engine.  The state dict has
checkpoint.Adam's keys and dtypes."""
import numpy as np

F = np.float32


def setup(n, beta=(0.9, 0.999)):
    """mgn_adam_init: zero moments, beta_t = the descriptor's (float) betas widened to double"""
    return {"mt": np.zeros(n, F), "vt": np.zeros(n, F), "beta_t": np.array([F(beta[0]), F(beta[1])], np.float64)}


def update(state, ps, g, eta=1e-3, beta=(0.9, 0.999), epsilon=1e-8):
    """-> (state', ps'): m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) (g g);  p <- p - ((m / c1) / (sqrt(v / c2) + eps)) eta"""
    b1, b2, eta, eps = F(beta[0]), F(beta[1]), F(eta), F(epsilon)
    omb1, omb2 = F(1) - b1, F(1) - b2
    g, ps = np.asarray(g, F), np.asarray(ps, F)
    bt = np.asarray(state["beta_t"], np.float64)
    c1, c2 = F(1.0 - bt[0]), F(1.0 - bt[1])
    mt = b1 * state["mt"] + omb1 * g
    vt = b2 * state["vt"] + omb2 * (g * g)
    dx = ((mt / c1) / (np.sqrt(vt / c2) + eps)) * eta
    out = ps - dx
    assert mt.dtype == vt.dtype == dx.dtype == out.dtype == F
    return {"mt": mt, "vt": vt, "beta_t": bt * np.array([b1, b2], np.float64)}, out


def synthetic_grads(n, seed):
    """magnitudes 1e-3 .. 1e3, either sign, with exact zeros mixed in (sqrt(0) + eps)"""
    rng = np.random.default_rng(seed)
    g = (10.0 ** rng.uniform(-3.0, 3.0, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    g[rng.random(n) < 0.05] = 0.0
    return g
