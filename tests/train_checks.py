"""Checks the training tests share (test infrastructure; numpy and the oracle only, no GPU): the bounds mgn_step is held to against the
float64 oracle, the per-tensor gradient comparison, and the ulp measure of an affine normaliser's values."""
import numpy as np

import mgn_oracle as orc

F32 = np.float32

TOL_LOSS = 1e-5      # relative
TOL_GRAD = 2e-4      # max|d| / max|ref| per parameter tensor (fp32 reductions over up to ~12k rows, 15 steps deep)


def check_grads(gs, ref, cfg, tol=TOL_GRAD):
    """Every parameter tensor within tol (max|d| / max|ref|, the tensor's own scale or 1e-3 of the whole gradient's).  The report names
    the worst tensor and, where the feature widths enter the model, the first layer of every encoder and the decoder's last layer."""
    h = cfg.get("hidden_layers", 2)
    width_tensors = ("enc_node.W1", "enc_edge.W1", "enc_edge2.W1", "decoder.W%d" % (h + 1), "decoder.b%d" % (h + 1))
    off, worst, widths = 0, ("", 0.0), {}
    for bname, tensors in orc.model_layout(cfg["Fn"], cfg["Fe"], cfg["O"], cfg["L"], h, cfg["mps"], cfg.get("Fe2")):
        for tname, shape in tensors:
            n = int(np.prod(shape))
            a, b = gs[off:off + n], ref[off:off + n]
            scale = max(np.abs(b).max(), 1e-3 * np.abs(ref).max())
            err = float(np.abs(a - b).max() / scale)
            if err > worst[1]:
                worst = (f"{bname}.{tname}", err)
            if f"{bname}.{tname}" in width_tensors:
                widths[f"{bname}.{tname}"] = err
            off += n
    assert off == ref.size
    assert worst[1] <= tol, (worst, widths)
    return worst


def affine_ulps(y, ref, x, scale, shift):
    """|y - ref| in ulps of the affine map's working magnitude (module docstring); returns the worst."""
    x, scale, shift = np.asarray(x, F32), np.asarray(scale, F32), np.asarray(shift, F32)
    mag = np.maximum(np.maximum(np.abs(x * scale), np.abs(shift)), np.maximum(np.abs(ref), np.abs(y)))
    return float((np.abs(y.astype(np.float64) - ref.astype(np.float64)) / np.spacing(mag.astype(F32)).astype(np.float64)).max())
