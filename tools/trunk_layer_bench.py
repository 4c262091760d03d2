#!/usr/bin/env python3
"""One bottleneck layer of the trunk, float32 path (split-K conv + reduction launch) vs the 16-bit small-tile kernel
(tools only).  Shapes: res4 2a / 2b / 2c and res3 2b at 4 images of 256 x 256 and 512 x 512."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from caesar_mrcnn_amd import ops
dev = torch.device("cuda:0")
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def spread(fn, batches=15, reps=20):
    """median, min, max (us per launch) over `batches` timed loops of `reps` launches."""
    ts = sorted(timed(fn, reps) for _ in range(batches))
    return ts[len(ts) // 2], ts[0], ts[-1]


def shortk_ab(json_path=None):
    """float32 res4 2c forward (BN, shortcut, ReLU, pre-BN output) and the data gradient of res4 2a through conv2d_dgrad_ep
    (residual + dy_out): the two-launch split-K plan (tuning key "sk64" = 0) against conv_fwd_sk64_kernel (1), same process.
    At 32 x 32 maps (M = 4096) the planner does not cut K (512 tiles of 64 x 128), so both columns time the same unsplit launch."""
    import json
    rows = []
    for nimg, hw in ((4, 16), (4, 32), (2, 16), (1, 16), (8, 16)):     # the last two: the ends of the kernel's default window
        M = nimg * hw * hw
        x = torch.randn(nimg, hw, hw, 256, device=dev)
        w = torch.randn(1, 1, 256, 1024, device=dev) * 0.05
        b = torch.zeros(1024, device=dev); sc = torch.rand(1024, device=dev) + 0.5; sh = torch.randn(1024, device=dev) * 0.1
        r = torch.randn(nimg, hw, hw, 1024, device=dev)
        out, z, dy = (torch.empty(nimg, hw, hw, 1024, device=dev) for _ in range(3))
        below_out = torch.relu(torch.randn(nimg, hw, hw, 1024, device=dev)); below_z = torch.randn(nimg, hw, hw, 1024, device=dev)
        mean = torch.randn(1024, device=dev); rstd = torch.rand(1024, device=dev) + 0.5
        sums = [torch.zeros(1024, device=dev) for _ in range(3)]
        legs = (("2c fwd  ", lambda: ops.conv2d(x, w, b, sc, sh, r, 1, "valid", 1, 1, out=out, z_out=z)),
                ("2a dgrad", lambda: ops.conv2d_dgrad_ep(x, w, "valid", below_out, below_z, sc, mean, rstd, sums[0], sums[1], sums[2], 1,
                                                         res=r, out=out, dy_out=dy)))
        for name, fn in legs:
            if fn() is None:                              # conv2d_dgrad_ep: no split-K plan at this size, the caller uses two calls
                rows.append({"M": M, "leg": name.strip(), "pair_us": None, "sk64_us": None})
                print("M=%5d %s 256->1024  no split-K plan: conv2d_dgrad_ep reports unsupported" % (M, name), flush=True)
                continue
            t = {}
            for key in (0, 1, 0, 1):                      # interleaved: each side twice, the better median kept
                ops.tuning_set("sk64", key)
                try:
                    s = spread(fn)
                finally:
                    ops.tuning_set("sk64", -1)
                if key not in t or s[0] < t[key][0]:
                    t[key] = s
            rows.append({"M": M, "leg": name.strip(), "pair_us": t[0], "sk64_us": t[1]})
            print("M=%5d %s 256->1024  pair %6.1f [%5.1f-%5.1f] us   sk64 %6.1f [%5.1f-%5.1f] us" % ((M, name) + t[0] + t[1]), flush=True)
    if json_path:
        with open(json_path, "w") as f:
            json.dump({"unit": "us per launch: median, min, max of 15 loops of 20 launches", "rows": rows}, f, indent=1)


if "--shortk" in sys.argv:
    i = sys.argv.index("--shortk")
    shortk_ab(sys.argv[i + 1] if i + 1 < len(sys.argv) else None)
    sys.exit(0)

os.environ["MRCNN_H16_SMALL"] = "1"
for hw in (16, 32, 64):
    for name, cin, cout, k in (("2a", 1024, 256, 1), ("2b", 256, 256, 3), ("2c", 256, 1024, 1)):
        x = torch.randn(4, hw, hw, cin, device=dev)
        w = torch.randn(k, k, cin, cout, device=dev) * 0.02
        b = torch.zeros(cout, device=dev); sc = torch.ones(cout, device=dev)
        out = torch.empty(4, hw, hw, cout, device=dev)
        t32 = timed(lambda: ops.conv2d(x, w, b, sc, b, None, 1, "same" if k == 3 else "valid", 1, out=out))
        line = "M=%5d %s %4d->%4d k%d  f32 %6.1f us" % (4 * hw * hw, name, cin, cout, k, t32)
        for dt in (torch.float16,):
            xh = x.to(dt); wf, wd = ops.weights_to_h16(w, dt)
            oh = torch.empty(4, hw, hw, cout, device=dev, dtype=dt)
            t16 = timed(lambda: ops.conv2d_h16(xh, wf, (k, k, cin, cout), b, sc, b, 1, "same" if k == 3 else "valid", 1, out=oh))
            gf = 2.0 * 4 * hw * hw * cin * cout * k * k / 1e9
            line += "   f16 small %6.1f us (%5.1f TFLOP/s)" % (t16, gf / t16 * 1e3)
        print(line, flush=True)
