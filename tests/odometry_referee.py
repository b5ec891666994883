"""NumPy referee of the visual-odometry contract (include/loopy_hip.h, "visual odometry"): the pyramid, one Gauss-Newton iteration and the
whole multi-scale estimate, in the operation order the header states, at a chosen precision (`dtype`, float64 by default; float32 is the
second precision of the whole-estimate yardstick).  Scalars that cross the C ABI as float are rounded to float32 first, as the library sees
them.  Besides the sums, an iteration returns the sums of the absolute values of their terms and the MARGIN SET: the pixels where fp32 and
fp64 may decide differently - within BOUNDARY_PX of a floor boundary, within TRUNC_M of the outlier truncation, or fed by a pyramid depth
that had a neighbour within DIFF_M of depth_diff."""
import numpy as np

K5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
BOUNDARY_PX, TRUNC_M, DIFF_M = 1e-4, 1e-5, 1e-5
PLANES = ('I', 'Vx', 'Vy', 'D', 'Ix', 'Iy', 'Dx', 'Dy')
F = np.diag([1.0, -1.0, -1.0, 1.0])
REC = 33


def f32(v):
    return float(np.float32(v))


def level0(color, depth, max_depth, dtype=np.float64):
    c, d = np.asarray(color, dtype=np.float32).astype(dtype), np.asarray(depth, dtype=np.float32).astype(dtype)
    k = [dtype(np.float32(v)) for v in (0.299, 0.587, 0.114)]
    I = (k[0] * c[..., 0] + k[1] * c[..., 1]) + k[2] * c[..., 2]
    D = np.where((d > 0) & (d <= dtype(f32(max_depth))), d, dtype(np.nan))
    return I.astype(dtype), D.astype(dtype)


def dilate(m, r):
    """True where any pixel within r (Chebyshev) is."""
    p = np.pad(m, r, mode='constant', constant_values=False)
    out = np.zeros_like(m)
    for a in range(2 * r + 1):
        for b in range(2 * r + 1):
            out |= p[a:a + m.shape[0], b:b + m.shape[1]]
    return out


def down(I, D, depth_diff, dtype=np.float64):
    """(I, D, margin) of the next level: margin = a neighbour within DIFF_M of the depth_diff decision."""
    H, W = I.shape
    h, w = H // 2, W // 2
    K = [dtype(v) for v in K5]
    p = np.pad(I, 2, mode='edge')
    t = np.zeros((H + 4, W), dtype=dtype)
    for k in range(5):
        t = t + K[k] * p[:, k:k + W]
    o = np.zeros((H, W), dtype=dtype)
    for r in range(5):
        o = o + K[r] * t[r:r + H]
    I2 = o[0:2 * h:2, 0:2 * w:2]
    diff = dtype(f32(depth_diff))
    q = np.pad(D, 2, mode='constant', constant_values=np.nan)
    c = D[0:2 * h:2, 0:2 * w:2]
    num, den, margin = np.zeros((h, w), dtype=dtype), np.zeros((h, w), dtype=dtype), np.zeros((h, w), dtype=bool)
    with np.errstate(invalid='ignore'):
        for r in range(5):
            for k in range(5):
                v = q[r:r + 2 * h:2, k:k + 2 * w:2]
                gap = np.abs(v - c)
                ok = gap <= diff
                wgt = K[r] * K[k]
                num = num + np.where(ok, wgt * v, dtype(0))
                den = den + np.where(ok, wgt, dtype(0))
                margin |= np.abs(gap.astype(np.float64) - float(diff)) < DIFF_M
        D2 = np.where(np.isfinite(c), num / np.where(den > 0, den, dtype(1)), dtype(np.nan))
    return I2.astype(dtype), D2.astype(dtype), margin


def sobel(P):
    p = np.pad(P, 1, mode='edge')
    e = P.dtype.type(0.125)
    two = P.dtype.type(2)
    with np.errstate(invalid='ignore'):
        dx = (((p[:-2, 2:] + two * p[1:-1, 2:]) + p[2:, 2:]) - ((p[:-2, :-2] + two * p[1:-1, :-2]) + p[2:, :-2])) * e
        dy = (((p[2:, :-2] + two * p[2:, 1:-1]) + p[2:, 2:]) - ((p[:-2, :-2] + two * p[:-2, 1:-1]) + p[:-2, 2:])) * e
    return dx, dy


def derive(I, D, K, dtype=np.float64):
    """The level's planes from its intensity and depth; K = (fx, fy, cx, cy) of the level."""
    h, w = I.shape
    fx, fy, cx, cy = (dtype(v) for v in K)
    yy, xx = np.mgrid[0:h, 0:w]
    Ix, Iy = sobel(I)
    Dx, Dy = sobel(D)
    bad = dilate(~np.isfinite(np.pad(D, 1, mode='edge')), 1)[1:-1, 1:-1]
    Dx, Dy = np.where(bad, dtype(np.nan), Dx), np.where(bad, dtype(np.nan), Dy)
    with np.errstate(invalid='ignore'):
        Vx, Vy = ((xx.astype(dtype) - cx) / fx) * D, ((yy.astype(dtype) - cy) / fy) * D
    return dict(I=I, Vx=Vx.astype(dtype), Vy=Vy.astype(dtype), D=D, Ix=Ix, Iy=Iy, Dx=Dx.astype(dtype), Dy=Dy.astype(dtype), K=tuple(float(v) for v in K))


def pyramid(color, depth, K, n_levels, max_depth=10.0, depth_diff=0.14, dtype=np.float64):
    """One dict per level: the eight planes, K, and three masks - mOwn (the pixel's own depth had a neighbour within DIFF_M of the depth_diff
    decision: what an iteration's margin set counts), mD (mOwn or fed by such a pixel of a finer level: the depth VALUE may differ between the
    precisions) and mG (a depth derivative that reads an mD pixel); the pyramid comparison leaves mD and mG out."""
    K = tuple(f32(v) for v in K)
    I, D = level0(color, depth, max_depth, dtype)
    mD = own = np.zeros(I.shape, dtype=bool)
    out = []
    for l in range(n_levels):
        if l > 0:
            I, D, own = down(I, D, depth_diff, dtype)
            h, w = I.shape
            mD = own | dilate(mD, 2)[0:2 * h:2, 0:2 * w:2]
            K = tuple(0.5 * v for v in K)
        lev = derive(I, D, K, dtype)
        lev['mOwn'], lev['mD'], lev['mG'] = own, mD, dilate(mD, 1)
        out.append(lev)
    return out


def level_from_planes(planes, K):
    """A level dict from [8, h, w] planes of the library (teacher-forced iterations): no pyramid margin."""
    lev = {name: np.asarray(planes[i]) for i, name in enumerate(PLANES)}
    lev['K'] = tuple(float(v) for v in K)
    lev['mOwn'] = lev['mD'] = lev['mG'] = np.zeros(lev['I'].shape, dtype=bool)
    return lev


def iteration(src, tgt, T, trunc=0.07, huber_i=0.1, huber_d=0.05, dtype=np.float64):
    """The sums of one iteration at one level.  Returns a dict: sums [29] (A upper triangle 21, b 6, loss, count) and abs [29] (the sums of
    the absolute values of the terms) in float64; margin (bool per pixel), n_margin, margin_abs [29] (the margin pixels' own absolute
    contributions); valid (bool per pixel)."""
    cast = lambda a: np.asarray(a).astype(dtype)
    fx, fy, cx, cy = (dtype(v) for v in src['K'])
    Tf = np.asarray(T, dtype=np.float64).astype(np.float32).astype(dtype)
    R, t = Tf[:3, :3], Tf[:3, 3]
    trunc, huber_i, huber_d = dtype(f32(trunc)), dtype(f32(huber_i)), dtype(f32(huber_d))
    h, w = src['I'].shape
    px, py, pz, Is = cast(src['Vx']), cast(src['Vy']), cast(src['D']), cast(src['I'])
    one = dtype(1)
    with np.errstate(all='ignore'):
        X = ((R[0, 0] * px + R[0, 1] * py) + R[0, 2] * pz) + t[0]
        Y = ((R[1, 0] * px + R[1, 1] * py) + R[1, 2] * pz) + t[1]
        Z = ((R[2, 0] * px + R[2, 1] * py) + R[2, 2] * pz) + t[2]
        ok0 = np.isfinite(pz) & (Z > 0)
        uf, vf = (fx * X) / Z + cx, (fy * Y) / Z + cy
        su, sv = uf + dtype(1.0 / 1024.0), vf + dtype(1.0 / 1024.0)
        u0, v0 = np.floor(su), np.floor(sv)
        inb = (u0 >= 0) & (u0 < w - 1) & (v0 >= 0) & (v0 < h - 1)
        near = (np.abs(su - np.rint(su)) < BOUNDARY_PX) | (np.abs(sv - np.rint(sv)) < BOUNDARY_PX)
        near &= (su > -1) & (su < w) & (sv > -1) & (sv < h)
        ui = np.clip(np.where(np.isfinite(u0), u0, 0), 0, w - 2).astype(np.int64)
        vi = np.clip(np.where(np.isfinite(v0), v0, 0), 0, h - 2).astype(np.int64)
        a, b = np.clip(uf - ui, 0, 1).astype(dtype), np.clip(vf - vi, 0, 1).astype(dtype)

        def bil(M):
            M = cast(M)
            return (one - b) * ((one - a) * M[vi, ui] + a * M[vi, ui + 1]) + b * ((one - a) * M[vi + 1, ui] + a * M[vi + 1, ui + 1])

        def any_tap(M):
            return M[vi, ui] | M[vi, ui + 1] | M[vi + 1, ui] | M[vi + 1, ui + 1]
        rD, hx, hy = bil(tgt['D']) - Z, bil(tgt['Dx']), bil(tgt['Dy'])
        fin = np.isfinite(rD) & np.isfinite(hx) & np.isfinite(hy)
        valid = ok0 & inb & fin & (np.abs(rD) <= trunc)
        margin = ok0 & near
        margin |= ok0 & inb & fin & (np.abs(np.abs(rD).astype(np.float64) - float(trunc)) < TRUNC_M)
        margin |= ok0 & (inb | near) & (src['mOwn'] | any_tap(tgt['mOwn']))
        rI, gx, gy = bil(tgt['I']) - Is, bil(tgt['Ix']), bil(tgt['Iy'])
        iz = one / Z

        def jac(qx, qy, depth):
            c0, c1 = (qx * fx) * iz, (qy * fy) * iz
            c2 = -((c0 * X + c1 * Y) * iz)
            J = [-(Z * c1) + Y * c2, Z * c0 - X * c2, -(Y * c0) + X * c1, c0, c1, c2]
            if depth:
                J[0], J[1], J[5] = J[0] - Y, J[1] + X, J[5] - one
            return J
        JI, JD = jac(gx, gy, False), jac(hx, hy, True)
        aI, aD = np.abs(rI), np.abs(rD)
        wI = np.where(aI <= huber_i, one, huber_i / aI).astype(dtype)
        wD = np.where(aD <= huber_d, one, huber_d / aD).astype(dtype)
        half = dtype(0.5)
        terms, absterms = [], []
        rows = [(i, j) for i in range(6) for j in range(i, 6)]
        for i, j in rows:
            p1, p2 = (wI * JI[i]) * JI[j], (wD * JD[i]) * JD[j]
            terms.append(p1 + p2)
            absterms.append(np.abs(p1) + np.abs(p2))
        for i in range(6):
            p1, p2 = (wI * JI[i]) * rI, (wD * JD[i]) * rD
            terms.append(p1 + p2)
            absterms.append(np.abs(p1) + np.abs(p2))
        loss = np.where(aI <= huber_i, half * rI * rI, huber_i * (aI - half * huber_i)) + \
            np.where(aD <= huber_d, half * rD * rD, huber_d * (aD - half * huber_d))
        terms += [loss, np.ones_like(loss)]
        absterms += [np.abs(loss), np.ones_like(loss)]
        # b with each residual replaced by the magnitudes it is the difference of: the scale of b's rounding error where the residuals cancel
        opI, opD = np.abs(rI + Is) + np.abs(Is), np.abs(rD + Z) + np.abs(Z)
        b_operands = np.array([float((np.abs(wI * JI[i]) * opI + np.abs(wD * JD[i]) * opD)[valid].astype(np.float64).sum()) for i in range(6)])
    sums, abss, margin_abs = np.zeros(29), np.zeros(29), np.zeros(29)
    n_margin = int(margin.sum())
    for k in range(29):
        tv = terms[k][valid]
        sums[k] = float(tv.sum(dtype=dtype)) if tv.size else 0.0
        av = absterms[k][valid].astype(np.float64)
        abss[k] = av.sum()
        if n_margin:
            am = absterms[k][margin].astype(np.float64)
            worst = av.max() if av.size else 0.0                # a margin pixel whose own terms are not finite counts as the worst valid one
            margin_abs[k] = np.where(np.isfinite(am), am, worst).sum()
    return dict(sums=sums, abs=abss, b_operands=b_operands, margin=margin, n_margin=n_margin, margin_abs=margin_abs, valid=valid, count=int(valid.sum()))


def rodrigues(wv):
    th = float(np.linalg.norm(wv))
    Kx = np.array([[0.0, -wv[2], wv[1]], [wv[2], 0.0, -wv[0]], [-wv[1], wv[0], 0.0]])
    ca, cb = (1.0, 0.5) if th < 1e-12 else (np.sin(th) / th, (1.0 - np.cos(th)) / (th * th))
    return np.eye(3) + ca * Kx + cb * (Kx @ Kx)


def solve_update(sums, T):
    """(T', |x|, flag) from the 29 sums: A x = -b by Cholesky in float64, T' = [exp(x0..2) | x3..5] T."""
    A = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[k]
            k += 1
    bvec = np.asarray(sums[21:27], dtype=np.float64)
    if sums[28] < 6 or not np.isfinite(A).all():
        return T, 0.0, 1
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return T, 0.0, 1
    x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -bvec))
    if not np.isfinite(x).all():
        return T, 0.0, 1
    dT = np.eye(4)
    dT[:3, :3], dT[:3, 3] = rodrigues(x[:3]), x[3:]
    return dT @ T, float(np.linalg.norm(x)), 0


def estimate(pyr_src, pyr_tgt, iters, trunc=0.07, huber_i=0.1, huber_d=0.05, T0=None, dtype=np.float64):
    """(T float64 [4,4], log): iters from the coarsest level to the finest; one log entry per iteration = the iteration's dict plus
    level, iter, step, flag and rec (the library's record)."""
    T = np.eye(4) if T0 is None else np.array(T0, dtype=np.float64)
    n, log = len(pyr_src), []
    for li, count in enumerate(iters):
        l = n - 1 - li
        for it in range(count):
            r = iteration(pyr_src[l], pyr_tgt[l], T, trunc, huber_i, huber_d, dtype)
            T, step, flag = solve_update(r['sums'], T)
            rec = np.zeros(REC)
            rec[0], rec[1], rec[2], rec[3] = l, it, r['sums'][28], r['sums'][27]
            rec[4:31], rec[31], rec[32] = r['sums'][:27], step, flag
            r.update(level=l, iter=it, step=step, flag=flag, rec=rec)
            log.append(r)
    return T, log


def compose(c2w_prev, T):
    """c2w of the source frame from the target frame's: c2w_prev F T F."""
    return np.asarray(c2w_prev, dtype=np.float64) @ F @ T @ F


def true_T(c2w_prev, c2w_cur):
    return F @ np.linalg.inv(np.asarray(c2w_prev, dtype=np.float64)) @ np.asarray(c2w_cur, dtype=np.float64) @ F
