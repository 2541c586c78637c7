"""What the per-row setup table of the one-wave-per-SIMD beam kernel costs at a given catalogue size: the build time of the table
(dm_build_g_table_kernel, first DM_G_TABLE=1 search minus a later one), the device memory it takes (hipMemGetInfo before / after)
and the search's kernel time with the table off and on.  usage: g_table_cost.py [users] [depth] [items]"""
import ctypes as C, os, sys, time, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dismember_amd import Engine, synth
U = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
depth = int(sys.argv[2]) if len(sys.argv) > 2 else 24
items = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
hip = C.CDLL("libamdhip64.so")


def free_bytes():
    f, t = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
    return f.value


rng = np.random.default_rng(synth.SEED)
tree = synth.make_tree(items, depth, rng)
seqs = synth.make_users(tree["leaf_ids"], U, 10, np.random.default_rng(1))
eng = Engine(0)
eng.load_tree(tree["codes"], tree["ids"], tree["is_leaf"], depth); eng.load_id_maps(tree["leaf_ids"], tree["leaf_codes"])
eng.load_weights_din_synthetic(128, (1 << (depth + 1)) - 1, synth.SEED, tree_depth=depth, rho=0.95)
d_seq = eng.dev_alloc(U * 40); d_ids = eng.dev_alloc(U * 800); d_sc = eng.dev_alloc(U * 800); d_cnt = eng.dev_alloc(U * 4)
eng.h2d(d_seq, seqs)


def search():
    eng.synchronize()
    t0 = time.perf_counter()
    eng.timing_reset()
    eng.tdm_beam_search_dev(d_seq, U, 10, 200, 200, d_ids, d_sc, d_cnt); eng.synchronize()
    n, ms = eng.timing_get_kind(0)
    return (time.perf_counter() - t0) * 1e3, ms / max(n, 1)


os.environ["DM_G_TABLE"] = "0"
search()                                   # the split copies exist after this one
wall_off, k_off = search()
f0 = free_bytes()
os.environ["DM_G_TABLE"] = "1"
wall_first, _ = search()                   # allocates and builds the table, then searches
f1 = free_bytes()
wall_on, k_on = search()
st = eng.g_table_state()
assert st["used_last"] and st["current"]
print("items %d depth %d: table %.2f GB (%d rows x 128 fp32); hipMemGetInfo free %.2f -> %.2f GB (delta %.2f GB)"
      % (items, depth, st["bytes"] / 1e9, st["bytes"] // 512, f0 / 1e9, f1 / 1e9, (f0 - f1) / 1e9))
print("first search with the table %.1f ms wall, later ones %.1f ms: allocation + build = %.1f ms" % (wall_first, wall_on, wall_first - wall_on))
print("search kernel, %d users: table off %.3f ms, table on %.3f ms (%s)" % (U, k_off, k_on, eng.last_beam_kernel()))
