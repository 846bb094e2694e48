"""Cases of the token-merging tests as data (tests/test_tome_ref_host.py, tests/test_gpu_tome_exact.py)."""

# (B, N, C, r, star): lattice keys (tests/tome_exact_ref.py) - the selection must be 100 % equal to the float64 reference
LATTICE = [
    (2, 8, 8, 4, False),           # smallest legal shape, the whole row is the scalar tail, everything merged
    (2, 136, 64, 17, False),       # N/2 = 68: tail of 4 columns
    (2, 137, 320, 40, False),      # odd N: trailing unpaired token
    (1, 1096, 64, 300, False),     # N/2 = 548: second 512-column trip plus tail
    (1, 4104, 64, 1000, False),    # N/2 = 2052 pairs: the sort holds four elements per thread
    (2, 64, 1536, 32, False),      # r = N/2 (no unmerged a token left), third channel vector of MAXV = 3
    (1, 512, 64, 256, True),       # star: every a token a copy of one b token, 257 rows into one destination (5 ballot rounds)
]
# the same, small enough for the dense adjoint map and the Python-loop emulations of the host self-test
LATTICE_SMALL = [c for c in LATTICE if c[1] <= 1100]

# (B, N, C, r): Gaussian keys and values, merged with the kernel's own selection and judged element-wise against float64
GAUSS = [
    (2, 8, 8, 4),
    (2, 136, 64, 17),
    (2, 137, 320, 40),
    (2, 64, 1536, 32),
    (1, 1096, 64, 300),
]

# adjoint: (B, N, C, r, star) - lattice keys fix the selection (large counts in the star case), Gaussian dy
ADJOINT = [
    (2, 136, 64, 17, False),
    (2, 137, 320, 40, False),      # odd N
    (2, 64, 1536, 32, False),
    (1, 512, 64, 256, True),       # star: weight 1 / 257
]

# refusals of gyre_op_tome_merge_ex: (what, overrides of the valid base call B=1 N=64 C=64 r=8, expected status)
MERGE_REFUSALS = [
    ("C = 1544", dict(C=1544), -1),
    ("N = 6", dict(N=6, r=1), -1),
    ("r = 0", dict(r=0), -1),
    ("ldvt < N - r", dict(ldvt=48), -1),
    ("N = 32776", dict(N=32776), -6),
    ("short workspace", dict(ws_bytes=4096), -4),
]
