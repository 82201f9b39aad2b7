"""Which gradients differ between two runs of the same eager train step (same weights, same batch)?

    python tools/determinism_probe.py [width] [B] [N] [--variant S|L|XL-MM] [--deterministic] [--runs R]

Default mode answers "most of them" (float atomics in the backward); with --deterministic (ops.deterministic_mode) every run
must give the same bits: the comparison is torch.equal, and the exit status is 1 if a tensor differs."""
import argparse, os, sys, torch
sys.path.insert(0, os.getcwd())
import amcontrast3d_amd
amcontrast3d_amd.activate()
from amcontrast3d_amd import configs, ops, synthetic
from openpoints.loss import build_criterion_from_cfg
from openpoints.models import build_model_from_cfg
from openpoints.utils import EasyConfig
ap = argparse.ArgumentParser()
ap.add_argument("width", nargs="?", type=int, default=16)
ap.add_argument("B", nargs="?", type=int, default=2)
ap.add_argument("N", nargs="?", type=int, default=2048)
ap.add_argument("--variant", default="S", choices=["S", "L", "XL-MM"])
ap.add_argument("--deterministic", action="store_true")
ap.add_argument("--runs", type=int, default=6)
args = ap.parse_args()
mm = args.variant == "XL-MM"
dev = "cuda:0"
torch.manual_seed(0)
c = EasyConfig()
c.update(configs.model_cfg_mm("XL", dropout=0, width=args.width, threshold=0.5) if mm else configs.model_cfg(args.variant, dropout=0, width=args.width))
model = build_model_from_cfg(c).to(dev).train()
cc = EasyConfig(); cc.update(configs.criterion_cfg_mm() if mm else configs.criterion_cfg()); crit = build_criterion_from_cfg(cc).to(dev)
aa = EasyConfig(); aa.update(configs.ambiguity_args_mm("s3dis") if mm else configs.ambiguity_args("s3dis"))
data = {k: torch.from_numpy(v).to(dev) for k, v in synthetic.make_batch(args.B, args.N, first_id=300).items()}
state = {k: v.clone() for k, v in model.state_dict().items()}
runs = []
with ops.deterministic_mode(args.deterministic):
    for r in range(args.runs):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        if mm:
            logits, stage, _ = model(dict(data))
            seg, _, _, reg = crit(logits, data["y"], stage, 13, None, aa)
            loss = seg + reg
        else:
            logits, stage = model(dict(data))
            loss = crit(logits, data["y"], stage, 13, None, aa)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
base = runs[0]
unequal = 0
for r, (lg, ls, g) in enumerate(runs[1:], 1):
    bad, differ = [], [n for n in g if not torch.equal(g[n], base[2][n])]
    for n in differ:
        d = float((g[n] - base[2][n]).abs().max())
        s = float(base[2][n].abs().max())
        if d > 1e-4 * max(s, 1e-6):
            bad.append((n, d, s))
    unequal += len(differ) + int(not torch.equal(lg, base[0])) + int(not torch.equal(ls, base[1]))
    print(f"run {r}: logits equal {torch.equal(lg, base[0])}, loss equal {torch.equal(ls, base[1])} (diff {abs(float(ls) - float(base[1])):.2e}), "
          f"gradient tensors not torch.equal: {len(differ)} of {len(g)}, off by > 1e-4 of their range: {len(bad)}")
    for n, d, s in bad[:12]:
        print(f"     {n:60s} diff {d:.3e} range {s:.3e}")
print(f"variant {args.variant} width {args.width} {args.B} x {args.N}, deterministic mode {'on' if args.deterministic else 'off'}: "
      f"{'every run has the same bits' if unequal == 0 else f'{unequal} tensors differ between runs'}")
sys.exit(1 if args.deterministic and unequal else 0)
