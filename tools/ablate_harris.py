"""Time k_harris<7> ablation variants on the GPU (diagnostic build: make ABLATIONS=1 and
SFMFEAT_LIB=<repo>/sfmfromscratch_amd/lib_diag/libsfmfeat.so).  The variants are interleaved
with the full kernel, round after round, so a drift of the box shows in the full kernel's spread.
usage: python tools/ablate_harris.py [rounds] [--levels]  (--levels: the four P-oct level sizes)"""
import ctypes, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sfmfromscratch_amd import _native
L = _native.load_library()
f = L.sfm_debug_time_harris
f.restype = ctypes.c_float
f.argtypes = [ctypes.c_int32] * 6
args = [a for a in sys.argv[1:] if a != "--levels"]
rounds = int(args[0]) if args else 1
sizes = [(1080 >> l, 1920 >> l) for l in range(4)] if "--levels" in sys.argv[1:] else [(1080, 1920)]
VARIANTS = [(0, "full"), (1, "no-hist"), (2, "window-1row"), (4, "no-barriers"), (5, "no-tap-loads")]
for r in range(rounds):
    for B, (H, W) in [(32, s) for s in sizes]:
        for abl, name in VARIANTS + [(0, "full")]:
            print(f"round {r} B={B} {H}x{W} {name:12s} {f(0, abl, B, H, W, 20):8.3f} ms", flush=True)
