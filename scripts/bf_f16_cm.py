"""The measurement behind the model constant c_m of the 16-bit tile path's certificate (bf_f16.hip,
DESIGN.md 4.6), on one GPU:

    python scripts/bf_f16_cm.py

Runs bf_query on the 16-bit tiles (BF_F16 = 2) over adversarial inputs with the re-rank's ratio sink set
(ggnn_debug_bf_f16_ratio_sink) and prints, per case, the largest

    |d_e - d_dir| / ((2D+8) 2^-24 (|q|^2 + |x|^2))

over every candidate the tile kernels kept: d_e is the tiles' expanded-form value, d_dir the re-rank's
direct form of the same pair, both float32.  d_dir is itself within (D+3) 2^-24 of the true distance, and
the two errors may cancel, so the figure estimates the model's error and does not bound it; the factor
four on top, the floor c_m >= 1 and the re-rank's run-time guard are what carry that.  The last line gives
the implied and the chosen c_m.  No value is subnormal in its type (the flag would send the call to the
scan and the sink would stay 0).  Nothing here is asserted anywhere."""
import json

import numpy as np
import torch

from ggnn_amd import _lib, ops

DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def data(kind, D, rng, n):
    x = rng.normal(size=(n, D))
    if kind == "offset1000":
        x = x + 1000
    if kind == "offset300":
        x = x + 300
    if kind == "decades":
        x = x * 10.0 ** rng.uniform(-1.5, 1.5, (n, 1))
    if kind == "alternating200":
        x = x + np.tile([200.0, -200.0], D // 2)
    x[np.abs(x) < 1e-4] = 0
    return x.astype(np.float32)


def main():
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    worst = (0.0, 0.0)
    try:
        _lib.lib().ggnn_debug_bf_f16_ratio_sink(word.data_ptr())
        for t in DT:
            for kind in ("normal", "offset1000", "offset300", "decades", "alternating200"):
                for D in (8, 128, 264, 960):
                    for K in (10, 100):
                        rng = np.random.default_rng(31)
                        b = torch.from_numpy(data(kind, D, rng, 4096)).cuda().to(DT[t])
                        q = torch.from_numpy(data(kind, D, rng, 256)).cuda().to(DT[t])
                        word.zero_()
                        with _lib.hooks(BF_F16=2):
                            resc = ops.bf_query(b, q, K, 0, rescanned=True)[2]
                        torch.cuda.synchronize()
                        ratio = float(word.view(torch.float32).item())
                        implied = ratio * (2 * D + 8) / (1.02 * (2.0625 * D + 24))
                        worst = max(worst, (implied, ratio))
                        print(json.dumps({"dtype": t, "data": kind, "D": D, "K": K, "ratio": round(ratio, 4),
                                          "implied_c_m": round(implied, 4), "n_rescanned": resc}), flush=True)
    finally:
        _lib.lib().ggnn_debug_bf_f16_ratio_sink(None)
    c_m = max(1.0, 2.0 ** np.ceil(np.log2(4 * worst[0])))
    print(json.dumps({"largest_implied_c_m": round(worst[0], 4), "at_ratio": round(worst[1], 4),
                      "four_times": round(4 * worst[0], 4), "c_m": c_m}))


if __name__ == "__main__":
    main()
