"""Solve batches (mnk_solve_batch_begin / _end) as the host sees them: 32 systems of order 512 (one merged launch: the host's
planning and launch rate is the bound) and 6 of order 11 192 (launches of four and two), quasi-definite LDL^T on one context.  Per
shape: wall time per batch (median of 5 blocks of 400 / 60 batches after 10 warm-ups, stream synchronized per block) and one
sha256 over all solutions, to compare two builds (record: profiles/solve_plan_ab.json).
usage: [MNK_LIBPATH=...] python tools/solve_batch_time.py"""
import hashlib, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import madnlp_jl_amd as mj
out = {}
for N, count, reps in ((512, 32, 400), (11192, 6, 60)):
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = mj.HipContext(0, stream=st.cuda_stream)
        g = torch.Generator(device="cuda").manual_seed(N)
        sols, rhs = [], []
        for i in range(count):
            R = torch.randn(N, 40, dtype=torch.float64, device="cuda", generator=g)
            A = R @ R.T
            A.diagonal().add_(float(N))
            A[2 * N // 3:, 2 * N // 3:].neg_()
            st.synchronize()
            M = mj.HipLinearSolver(A, ctx=ctx, opt=mj.HipSolverOptions(lapack_algorithm=mj.LDL))
            M.factorize()
            sols.append(M)
            rhs.append(torch.randn(N, dtype=torch.float64, device="cuda", generator=g))
        xs = [b.clone() for b in rhs]
        def batch():
            with mj.solve_batch():
                for M, x in zip(sols, xs):
                    M.solve_linear_system(x)
        for _ in range(10):
            batch()
        st.synchronize()
        blocks = []
        for blk in range(5):
            torch._foreach_copy_(xs, rhs); st.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                batch()
            st.synchronize()
            blocks.append((time.perf_counter() - t0) / reps * 1e3)
        torch._foreach_copy_(xs, rhs); batch(); st.synchronize()
        h = hashlib.sha256(b"".join(x.cpu().numpy().tobytes() for x in xs)).hexdigest()[:16]
        out[f"solve_batch_{count}x{N}_ms_median_of_5_blocks"] = sorted(blocks)[2]
        out[f"solve_batch_{count}x{N}_sha"] = h
        for M in sols:
            M.close()
        ctx.close()
print(json.dumps(out))
