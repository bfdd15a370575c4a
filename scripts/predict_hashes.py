"""SHA-256 of every output of a fixed, seeded list of prediction calls (ops.predict_mask, predict_mask_views, predict_mask_tiles:
csrc/predict.hip), one line per output.  Every output is an integer map, so two builds of the library compute the same thing
exactly when the two listings are equal:
    python scripts/predict_hashes.py [--lib PATH/libasis_hip.so] > hashes.txt
The list holds all three ops; every instance of the kernels (load width V in {4, 2, 1} from C and the address of the first map,
class bucket CB in {4, 8, 16} from C: C = 1..16 with the first map 0, 1 and 2 floats off a 16-byte boundary); plain and mirrored
maps; both blends; confidence, overlay and counts on and off; widths with short and unaligned quads; and the workloads of
scripts/bench_predict_views.py and scripts/bench_predict_tiles.py."""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def randn(g, shape, dev, off=0):
    """3 * randn on the device, ``off`` floats after a 16-byte boundary."""
    t = 3 * torch.randn(shape, generator=g)
    flat = torch.zeros(t.numel() + 4, device=dev)
    assert flat.data_ptr() % 16 == 0
    out = flat[off:off + t.numel()].view(shape)
    out.copy_(t)
    return out


def calls(dev):
    """-> (name, thunk) pairs; a thunk returns a tensor or a tuple of tensors."""
    from adaptersis_amd import ops
    from adaptersis_amd import predict as P
    from adaptersis_amd.tools import frame_resize as FR
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_predict_views import view_sizes
    g = torch.Generator().manual_seed(20261019)
    u8 = lambda hi, shape: torch.randint(0, hi, shape, generator=g, dtype=torch.uint8).to(dev)
    two = [(0, 0, 16, 10, False), (0, 6, 16, 10, True)]
    for C in range(1, 17):
        for off in (0, 1, 2):                                                    # every (V, CB): small maps, short quads
            a, b = randn(g, (2, 5, 7, C), dev, off), randn(g, (2, 6, 4, C), dev)
            yield f"mask C={C} off={off}", lambda a=a: ops.predict_mask(a, (9, 13))
            yield f"views C={C} off={off}", lambda a=a, b=b: ops.predict_mask_views([a, b], (9, 13), flips=[False, True], confidence=True)
            for blend in ops.PREDICT_BLENDS:
                yield (f"tiles C={C} off={off} {blend}",
                       lambda a=a, b=b, blend=blend: ops.predict_mask_tiles([a, b], two, 16, (9, 13), blend=blend, confidence=True))
    tiles = P.plan_tiles(80, 48, 32, True, True)                                 # 10 tiles: 2 x 2 windows and the context, each twice
    for C in (2, 3, 8, 10, 11, 16):
        for H, W in ((131, 203), (64, 320), (9, 7), (9, 1)):                     # unaligned rows, whole quads, tails
            enc = torch.from_numpy(FR.ENCODE_ENDOVIS2017[:min(C, 8)].copy()) if C <= 8 else None
            extra = dict(frames=u8(256, (2, H, W, 3)), palette=u8(256, (C, 3)), alpha=u8(256, (C,)), target=u8(8, (2, H, W)) * 32,
                         lut=FR.LUT_MULTI)
            views = [randn(g, (2, h, w, C), dev) for h, w in ((24, 30), (31, 27), (17, 19), (42, 42))]
            maps = [randn(g, (2, 17 + k, 19 - k, C), dev) for k in range(len(tiles))]
            for tag, kw in (("plain", {}), ("all", extra)):
                yield f"mask C={C} {H}x{W} {tag}", lambda v=views[0], kw=kw, enc=enc, s=(H, W): ops.predict_mask(v, s, enc, **kw)
                yield (f"views C={C} {H}x{W} {tag}", lambda v=views, kw=kw, enc=enc, s=(H, W):
                       ops.predict_mask_views(v, s, enc, flips=[False, True, True, False], confidence=bool(kw), **kw))
                for blend in ops.PREDICT_BLENDS:
                    yield (f"tiles C={C} {H}x{W} {blend} {tag}", lambda m=maps, kw=kw, enc=enc, s=(H, W), blend=blend:
                           ops.predict_mask_tiles(m, tiles, 80, s, enc, blend=blend, ramp=16, confidence=bool(kw), **kw))
    for h in (147, 168):                                                         # bench_predict_views.py
        for C in (2, 8):
            for K in (2, 6):
                gb = torch.Generator().manual_seed(C * 100 + K)
                sizes = view_sizes(h, K)
                views = [(3 * torch.randn((12, s, s, C), generator=gb)).to(dev) for s in sizes for _ in (0, 1)]
                enc = torch.from_numpy(FR.ENCODE_ENDOVIS2017[:C].copy()).to(dev)
                yield (f"bench views {h} C={C} K={K}", lambda v=views, enc=enc, n=len(sizes):
                       ops.predict_mask_views(v, (1080, 1920), enc, flips=[False, True] * n))
    for H, W in ((1024, 1280), (1080, 1920)):                                    # bench_predict_tiles.py
        for C in (2, 8, 11):
            for context, flip in ((False, False), (True, True)):
                tl = P.plan_tiles(1176, 588, 392, context, flip)
                gb = torch.Generator().manual_seed(C * 100 + len(tl))
                maps = [(3 * torch.randn((4, 147, 147, C), generator=gb)).to(dev) for _ in tl]
                enc = (torch.arange(C, dtype=torch.uint8) * 23).to(dev)
                yield (f"bench tiles {H}x{W} C={C} K={len(tl)}", lambda m=maps, tl=tl, enc=enc, s=(H, W):
                       ops.predict_mask_tiles(m, tl, 1176, s, enc, blend="ramp", ramp=196))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the shared library to load instead of the tree's own")
    a = ap.parse_args()
    if a.lib:
        from adaptersis_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    n = 0
    for name, thunk in calls(torch.device("cuda:0")):
        out = thunk()
        for k, t in enumerate(out if isinstance(out, tuple) else (out,)):
            print(f"{hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}  {name} [{k}] {t.dtype} {list(t.shape)}")
            n += 1
    print(f"# {n} outputs", file=sys.stderr)
