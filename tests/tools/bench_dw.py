"""Timing of nm_weight_grad at the training shapes (fine network of a 2048-ray batch: 393 216 samples), and a SHA-256 of dW | db
per shape for seeded operands (those four and one 64 x 64 product): two builds that print the same hashes reduce bit for bit alike."""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from nerfmeshes_amd import hip_ops, synthetic as S, train_ops as T
kw = dict(num_layers=8, hidden_size=256, skip_step=4, num_encoding_fn_xyz=10, num_encoding_fn_dir=4)
mlp = hip_ops.HipMLP(S.make_scene_weights(**kw), kw, "cuda")
n = 2048 * 192
out = {}
torch.manual_seed(0)
for o, s, i in ((256, 256, 256), (256, 64, 63), (128, 256, 256), (128, 64, 27), (64, 64, 64)):
    d = torch.randn(n, o, device="cuda"); a = torch.randn(n, s, device="cuda")
    dw, db = T._weight_grad(mlp, d, a, i); torch.cuda.synchronize()
    sha = hashlib.sha256(dw.cpu().numpy().tobytes() + db.cpu().numpy().tobytes()).hexdigest()
    if o == 64:
        out[f"{o}x{s}"] = {"sha256": sha}
        continue
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(5)]
    for x, y in ev:
        x.record(); T._weight_grad(mlp, d, a, i); y.record()
    torch.cuda.synchronize()
    ms = min(x.elapsed_time(y) for x, y in ev)
    out[f"{o}x{s}"] = {"sha256": sha, "ms": ms, "tflops_on_padded_shape": 2.0 * n * o * s / (ms * 1e-3) / 1e12,
                       "GBps_operands": 4.0 * n * (o + s) / (ms * 1e-3) / 1e9}
print(json.dumps(out))
