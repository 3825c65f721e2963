"""numpy restatement of the csim_ensemble_perturb block of include/csim.h (items 1 - 7), written from the text alone:
Philox4x32-10 in uint64 arithmetic, the AS241 normal quantile with the library's logarithm, the smoothing taps, and the
perturbation fields.  tests/test_ensemble_perturb_host.py pins items 1 - 3 to the library bit for bit and to
independent references; tests/test_gpu_ensemble_perturb.py uses items 4 - 7 as the reference of the kernel."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox(c, k):
    """c: four arrays (or scalars) of counter words, k: two key words; four uint64 arrays holding 32-bit words"""
    c = [np.asarray(x, dtype=np.uint64) for x in c]
    k0, k1 = np.asarray(k[0], dtype=np.uint64), np.asarray(k[1], dtype=np.uint64)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & U32, (p0 >> S32) ^ c[3] ^ k1, p0 & U32]
        k0, k1 = (k0 + np.uint64(W0)) & U32, (k1 + np.uint64(W1)) & U32
    return c


A = [3.3871328727963666080e0, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
     4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3]
B = [1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3, 2.1213794301586595867e4,
     3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3]
C = [1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
     1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4]
D = [1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
     1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9]
E = [6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
     2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7]
F = [1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
     7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15]
LN2 = float.fromhex("0x1.62e42fefa39efp-1")  # 0x3FE62E42FEFA39EF
SQRT_HALF = float(np.sqrt(0.5))


def horner(co, x):
    r = np.full_like(x, co[7])
    for n in range(6, -1, -1):
        r = r * x + co[n]
    return r


def log_restated(t):
    m, e = np.frexp(t)
    small = m < SQRT_HALF
    m = np.where(small, m * 2.0, m)
    e = np.where(small, e - 1, e).astype(np.float64)
    s = (m - 1.0) / (m + 1.0)
    w = s * s
    p = np.full_like(w, 1.0 / 23.0)
    for n in range(21, 0, -2):
        p = p * w + 1.0 / n
    return e * LN2 + 2.0 * (s * p)


def uniform_from_bits(bits):
    k = np.asarray(bits, dtype=np.uint64) >> np.uint64(12)
    return (k.astype(np.float64) + 0.5) * 2.0 ** -52


def normal_from_bits(bits):
    u = np.atleast_1d(uniform_from_bits(bits))
    q = u - 0.5
    r = 0.180625 - q * q
    centre = q * horner(A, r) / horner(B, r)
    t = np.where(q < 0, u, 1.0 - u)
    rr = np.sqrt(-log_restated(t))
    with np.errstate(all="ignore"):  # both tails are evaluated everywhere and selected
        tail = np.where(rr <= 5.0, horner(C, rr - 1.6) / horner(D, rr - 1.6), horner(E, rr - 5.0) / horner(F, rr - 5.0))
    tail = np.where(q < 0, -tail, tail)
    return np.where(np.abs(q) <= 0.425, centre, tail)


def gc(z):
    near = ((((-0.25 * z + 0.5) * z + 0.625) * z - 5.0 / 3.0) * z) * z + 1.0
    with np.errstate(all="ignore"):
        far = ((((z / 12.0 - 0.5) * z + 0.625) * z + 5.0 / 3.0) * z - 5.0) * z + 4.0 - 2.0 / (3.0 * z)
    v = np.where(z <= 1.0, near, np.where(z < 2.0, far, 0.0))
    return np.maximum(v, 0.0)


def radius(d, c, n, periodic):
    if c == 0:
        return 0
    clip = (n - 1) // 2 if periodic else n - 1
    a = 0
    while a + 1 <= clip and float(a + 1) * d < 2.0 * c:
        a += 1
    return a


def taps(d, c, n, periodic):
    R = radius(d, c, n, periodic)
    if c == 0:
        return np.array([1.0])
    g = gc(np.abs(np.arange(-R, R + 1)).astype(np.float64) * d / c)
    S = 0.0
    for v in g:
        S = S + v * v
    return g / np.sqrt(S)


def white(seed, draw, k, L):
    """w_k(L) of item 5 for an array of lattice indices L (uint64)"""
    L = np.asarray(L, dtype=np.uint64)
    n = L >> np.uint64(1)
    o = philox([n & U32, n >> S32, np.full_like(n, k), np.full_like(n, draw)], [seed & 0xFFFFFFFF, seed >> 32])
    odd = (L & np.uint64(1)).astype(bool)
    lo = np.where(odd, o[2], o[0])
    hi = np.where(odd, o[3], o[1])
    return normal_from_bits(lo | (hi << S32)).reshape(L.shape)


def axis_periodic(bc):
    return bc[0] == 2 and bc[1] == 2, bc[2] == 2 and bc[3] == 2


def field(seed, draw, k, nx, ny, dx, dy, corr_len, bc):
    """p_k of items 4 - 6 on the interior, shape (ny, nx)"""
    perx, pery = axis_periodic(bc)
    tx, ty = taps(dx, corr_len, nx, perx), taps(dy, corr_len, ny, pery)
    Rx, Ry = len(tx) // 2, len(ty) // 2
    Px = nx if perx else nx + 2 * Rx
    Py = ny if pery else ny + 2 * Ry
    b, a = np.meshgrid(np.arange(Py, dtype=np.uint64), np.arange(Px, dtype=np.uint64), indexing="ij")
    w = white(seed, draw, k, b * np.uint64(Px) + a)
    i = np.arange(nx)
    hx = np.zeros((Py, nx))
    for o in range(-Rx, Rx + 1):
        cols = (i + o) % nx if perx else i + o + Rx
        hx = hx + tx[o + Rx] * w[:, cols]
    j = np.arange(ny)
    p = np.zeros((ny, nx))
    for o in range(-Ry, Ry + 1):
        rows = (j + o) % ny if pery else j + o + Ry
        p = p + ty[o + Ry] * hx[rows, :]
    return p


def perturb(X, seed, draw, sigma, corr_len, centered, t, dx, dy, bc):
    """item 7 on members x (ny+2) x (nx+2): the state after csim_ensemble_perturb"""
    X = X.copy()
    Bm, ny, nx = X.shape[0], X.shape[1] - 2, X.shape[2] - 2
    if sigma == 0:
        return X
    ks = [k for k in range(Bm) if k != t]
    P = [field(seed, draw, k, nx, ny, dx, dy, corr_len, bc) for k in ks]
    if centered:
        s = np.zeros((ny, nx))
        for p in P:
            s = s + p
        pbar = s / float(len(ks))
        P = [p - pbar for p in P]
    for k, p in zip(ks, P):
        X[k, 1:-1, 1:-1] = X[k, 1:-1, 1:-1] + sigma * p
    return X
