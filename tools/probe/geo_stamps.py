"""Phase timings of the fused geometry kernels (csrc/grid_geometry.hip) from in-kernel wall-clock stamps.
Builds its own copy of the translation unit with -DOCOCC_GEO_STAMPS (the product library carries no stamps) and calls
it through ctypes on the benchmark batch (OCOCC_GEO_STAMPS_LIB: a copy built beforehand, with the same flags).  The
emit kernel's workgroups are stamped per role: row workgroups (grid, slice) first, point workgroups (grid, part) behind.
Run on the GPU box: python tools/probe/geo_stamps.py [slices]"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
csrc = os.path.join(ROOT, 'objectcentricocccompletion_amd', 'csrc')
slices = int(sys.argv[1]) if len(sys.argv) > 1 else 12
so = os.environ.get('OCOCC_GEO_STAMPS_LIB')
if not so:
    so = '/tmp/libgeo_stamps.so'
    subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '-fPIC', '-shared', '--offload-arch=gfx950', '-DOCOCC_GEO_STAMPS',
                    os.path.join(csrc, 'grid_geometry.hip'), os.path.join(csrc, 'grid_unique.hip'), os.path.join(csrc, 'capi.hip'),
                    os.path.join(csrc, 'sparse_conv_sorted.hip'),   # (the geometry call launches the order's placing pass)
                    '-o', so], check=True)
lib = ctypes.CDLL(so)
from objectcentricocccompletion_amd import _lib as L  # noqa: E402  (argument helpers only)
from objectcentricocccompletion_amd.occ_encoder import synthetic_object_grids  # noqa: E402

dev = torch.device('cuda:0')
B, P = 64, 2000
xyz, feats, bidx = synthetic_object_grids(B, P, seed=0, device=dev)
n, c, cap = B * P, 16, B * P
I3, F3, F6 = ctypes.c_int32 * 3, ctypes.c_float * 3, ctypes.c_float * 6
lib.ococc_object_grid_geometry_workspace_bytes.restype = ctypes.c_int64
lib.ococc_object_grid_geometry_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32, I3, ctypes.c_int32]
nbytes = lib.ococc_object_grid_geometry_workspace_bytes(n, B, I3(40, 40, 40), slices)
T = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
ws, coors, inv, counts = T((nbytes,), torch.uint8), T((cap, 4), torch.int32), T((n,), torch.int32), T((cap,), torch.int32)
out, out16, meta = T((cap, c), torch.float32), T((cap, c), torch.bfloat16), T((2,), torch.int32)
nbr, mask, pairs, num = T((27, cap), torch.int32), T(((cap + 15) // 16,), torch.int32), T((27, 2, cap), torch.int32), T((27,), torch.int32)
pparts = min(slices, 4)                                 # point workgroups per grid: one per kernel-A workgroup
nblocks = B * slices + B * pparts + 64                  # row, point and padding workgroups of the emit launch
stamps = torch.zeros((nblocks * 16,), dtype=torch.int64, device=dev)
lib.ococc_geo_set_stamps.argtypes = [ctypes.c_void_p]
assert lib.ococc_geo_set_stamps(stamps.data_ptr()) == 0
vp = ctypes.c_void_p
# (the entry the benchmark step takes: with the neighbour-pattern order, its placing pass launched by the same call)
lib.ococc_object_grid_geometry_order_f32.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int64, vp, ctypes.c_int32, F3, F6, ctypes.c_int32, I3,
                                                     ctypes.c_int32, vp, ctypes.c_int64] + [vp] * 11 + [ctypes.c_int64] + [vp] * 4 + \
                                                    [ctypes.c_int32, ctypes.c_int32, vp]
lib.ococc_subm_row_order_counter_bytes.restype = ctypes.c_int64
counters = torch.zeros((lib.ococc_subm_row_order_counter_bytes(),), dtype=torch.uint8, device=dev)
rowrec, rec, hdr = T((cap, 4), torch.int32), T((cap, 4), torch.int32), T((8,), torch.int32)
from objectcentricocccompletion_amd.spconv.ops import SORTED_TILES  # noqa: E402


def run():
    rc = lib.ococc_object_grid_geometry_order_f32(xyz.data_ptr(), 3, bidx.data_ptr(), n, feats.data_ptr(), c, F3(0.2, 0.2, 0.2),
                                            F6(-4, -4, -4, 4, 4, 4), B, I3(40, 40, 40), slices, coors.data_ptr(), cap,
                                            inv.data_ptr(), counts.data_ptr(), out.data_ptr(), out16.data_ptr(),
                                            meta.data_ptr(), meta.data_ptr() + 4, nbr.data_ptr(), mask.data_ptr(),
                                            pairs.data_ptr(), num.data_ptr(), ws.data_ptr(), nbytes, counters.data_ptr(),
                                            rowrec.data_ptr(), rec.data_ptr(), hdr.data_ptr(), SORTED_TILES[0], SORTED_TILES[1], None)
    assert rc == 0, rc


for _ in range(5):
    run()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    run()
e1.record()
torch.cuda.synchronize()
print('geometry with the order, us per call:', round(e0.elapsed_time(e1) / 20 * 1e3, 1), ' voxels', int(meta[0]))
st = stamps.cpu().numpy().reshape(-1, 16).astype(np.float64) / 100.0   # s_memrealtime ticks at 100 MHz -> us
A = st[:B * min(slices, 4)]
names_a = ['zero+segments', 'point pass', 'scan+bitmap out', 'neighbour counts']
print('kernel A (median over workgroups, us):', {nm: round(float(np.median(A[:, i + 1] - A[:, i])), 2) for i, nm in enumerate(names_a)},
      'whole', round(float(A[:, 4].max() - A[:, 0].min()), 2))
med = lambda x: round(float(np.median(x)), 2)
Rk = st[:B * slices]                                    # row role: stamps 5 6 (11 12 13 14: last round) 7 15
Rk = Rk[Rk[:, 11] > 0]                                  # (slices with rows)
print('emit, row role (median over workgroups, us):',
      {'bitmap, bases in': med(Rk[:, 6] - Rk[:, 5]), 'row loop': med(Rk[:, 7] - Rk[:, 6]),
       'order atomics back, records patched': med(Rk[:, 15] - Rk[:, 7]), 'chain': med(Rk[:, 15] - Rk[:, 5])},
      'longest', round(float((Rk[:, 15] - Rk[:, 5]).max()), 2))
print('  row loop detail (last round): cells', med(Rk[:, 11] - Rk[:, 6]), 'table, counts, records', med(Rk[:, 12] - Rk[:, 11]),
      'masks', med(Rk[:, 13] - Rk[:, 12]), 'prefix', med(Rk[:, 14] - Rk[:, 13]), 'pairs', med(Rk[:, 7] - Rk[:, 14]))
Pk = st[B * slices:B * slices + B * pparts]             # point role: stamps 5 6 8 9 10
print('emit, point role (median over workgroups, us):',
      {'codes, part bitmap, base in': med(Pk[:, 6] - Pk[:, 5]), 'inv and first arrivals': med(Pk[:, 8] - Pk[:, 6]),
       'later arrivals': med(Pk[:, 9] - Pk[:, 8]), 'means': med(Pk[:, 10] - Pk[:, 9]), 'chain': med(Pk[:, 10] - Pk[:, 5])},
      'longest', round(float((Pk[:, 10] - Pk[:, 5]).max()), 2))
both = np.concatenate([Rk[:, [5, 15]], Pk[:, [5, 10]]])
print('emit, first start to last end over both roles (us):', round(float(both[:, 1].max() - both[:, 0].min()), 2),
      ' point role starts behind the first row workgroup by (median, us)', med(Pk[:, 5] - Rk[:, 5].min()))
