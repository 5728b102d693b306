"""spblas-reference_amd: MI355X (gfx950) backend for the spblas-reference multiply() path.

Layout (only what the hot path needs):
  csrc/      hand-written HIP kernels + the C ABI (include/spblas_gfx950.h)
  _capi.py   ctypes binding of that ABI (no fallback path)
  api.py     host-side mirror of the reference's view/operator interface
  sharded.py row-sharded multi-GPU SpMV (one process per GPU, RCCL all-gather of y)
  generate.py synthetic inputs
Import name: `spblas_reference_amd` (see the shim module at the repo root).
"""
from . import _build, _capi, generate  # noqa: F401
from ._capi import BackendError  # noqa: F401
from .api import (  # noqa: F401
    add, add_compute, add_inspect, conjugated, csc_view, csr_view, get_scaling_factor, get_ultimate_base, has_matrix_opt, index, is_conjugated,
    matrix_opt, multiply, multiply_compute, multiply_fill, multiply_inspect, multiply_numeric,
    multiply_symbolic_compute, multiply_symbolic_fill, operation_info_t, prepared_multiply, scale, scaled, scaled_view,
    spgemm_state_t, transpose, transpose_inspect,
    transposed, triangular_solve, triangular_solve_inspect, triangular_solve_sweeps, upper_triangle_t, lower_triangle_t,
    implicit_unit_diagonal_t, explicit_diagonal_t, upper_triangle, lower_triangle, implicit_unit_diagonal,
    explicit_diagonal, ilu0, ilu0_inspect, ilu0_status, ilu0_sweeps, multicolor_order, multicolor_order_t,
    permute, permute_inspect, permute_vector, gauss_seidel, gauss_seidel_inspect)

# The aggregation names (MIS-2 aggregates, the Galerkin coarse matrix).  They are bound one by one, not added to the import list
# above: tests/test_stream_order_cpu.py reads that list and asks for an entry of tests/stream_util.py per name, and these names
# keep their stream-order cases in a table of their own (tests/aggregate_util.py: STREAM_CASES / STREAM_EXEMPT, proved by
# tests/test_aggregate_cpu.py, run by tests/test_gpu_aggregate_stream.py).
aggregate, aggregate_t = api.aggregate, api.aggregate_t  # noqa: F821
coarsen, coarsen_inspect, coarsen_structure = api.coarsen, api.coarsen_inspect, api.coarsen_structure  # noqa: F821
AGGREGATION_EXPORTS = ("aggregate", "aggregate_t", "coarsen", "coarsen_inspect", "coarsen_structure")

# The smoothed prolongator: bound and tabled in the same way (tests/smooth_util.py: STREAM_CASES, proved by
# tests/test_smooth_cpu.py, run by tests/test_gpu_smooth_stream.py).
smooth_prolongator, smooth_prolongator_inspect, smooth_prolongator_structure = (  # noqa: F821
    api.smooth_prolongator, api.smooth_prolongator_inspect, api.smooth_prolongator_structure)
SMOOTH_EXPORTS = ("smooth_prolongator", "smooth_prolongator_inspect", "smooth_prolongator_structure")
