"""Host cost of the partner draw, no GPU: pcgmix_partner_permutation_i64 at B = 256 with the benchmark's
label layout (synthetic.make_batch(256, 4, 5000, sample_rate=2000, seed=0)), a 50/50 and a 90/10 layout,
10 000 calls each, five repeats, ns per call.  The call seeds Random(step) itself (about 1,870 dependent
steps, the same on every tree), so the difference between two trees is the draw's.
   python profiles/probes/partner_draw_time.py            (PCGMIX_PROBE_LIB=<other tree's .so> for an A/B)"""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import pcgmix_amd  # noqa: F401
from pcgmix_amd import _lib, synthetic
if os.environ.get("PCGMIX_PROBE_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["PCGMIX_PROBE_LIB"])
lib = _lib.load()
B, CALLS = 256, 10000
rs = np.random.RandomState(1)
layouts = {
    "bench": synthetic.make_batch(B, 4, 5000, sample_rate=2000, seed=0)[2],
    "50/50": rs.permutation(np.arange(B) % 2),
    "90/10": rs.permutation((np.arange(B) < B // 10).astype(np.int64)),
}
print("library:", os.environ.get("PCGMIX_PROBE_LIB") or "product", flush=True)


def seeding(n):          # Random(step).uniform(0, 1): the seeding and the first regeneration, no draw
    lib.pcgmix_py_uniform01.restype = ctypes.c_double
    t0 = time.perf_counter()
    for step in range(n):
        lib.pcgmix_py_uniform01(ctypes.c_uint64(step))
    return (time.perf_counter() - t0) / n * 1e9


seeding(1000)
print("seeding alone (pcgmix_py_uniform01) ns/call: %s" % " ".join("%.0f" % seeding(CALLS) for _ in range(3)),
      flush=True)
for name, labels in layouts.items():
    keys = list(dict.fromkeys(int(v) for v in labels))           # first appearance
    gid = np.array([keys.index(int(v)) for v in labels], dtype=np.int32)
    mix = np.empty(B, dtype=np.int64)
    fn, g, m, k = lib.pcgmix_partner_permutation_i64, gid.ctypes.data, mix.ctypes.data, len(keys)

    def region(n):
        t0 = time.perf_counter()
        for step in range(n):
            fn(g, B, k, step, m)
        return (time.perf_counter() - t0) / n * 1e9

    region(1000)
    sizes = np.bincount(gid).tolist()
    print("%-6s groups %-12s ns/call: %s" % (name, sizes, " ".join("%.0f" % region(CALLS) for _ in range(5))),
          flush=True)
