"""The reference of the recursive-filter tests (test_sosfilt_host.py,
test_sosfilt_gpu.py): the recurrence of scipy.signal.sosfilt in long double,
a float64 run of the same recurrence (the error a sequential filter has
anyway), a numpy model of the time-parallel decomposition, and the test
filters' coefficients as literals, so that no test needs scipy.

The literals are what scipy.signal gives for: butter(8, 0.2), butter(6, [0.2,
0.3], "band"), cheby1(8, 1, 0.3, "high"), ellip(8, 0.1, 80, 0.05), butter(8,
0.01), butter(2, 0.001), butter(12, 0.002), each with output="sos".
"""
import numpy as np

LD = np.longdouble

TILE, E = 4096, 16

FILTERS = {k: np.array(v, dtype=np.float64) for k, v in {
    "butter8_0.2": [
        [2.395964410377617e-05, 4.791928820755234e-05, 2.395964410377617e-05, 1.0, -1.0263514742610553, 0.26864019099379005],
        [1.0, 2.0, 1.0, 1.0, -1.0868584613628944, 0.343430940165366],
        [1.0, 2.0, 1.0, 1.0, -1.2197253651240232, 0.5076634651740437],
        [1.0, 2.0, 1.0, 1.0, -1.4515795942478362, 0.794251053241888],
    ],
    "butter6_band": [
        [8.57655707325942e-06, 1.715311414651884e-05, 8.57655707325942e-06, 1.0, -1.182328318285603, 0.7252013970802744],
        [1.0, 2.0, 1.0, 1.0, -1.2982434320949163, 0.7449703925047285],
        [1.0, 2.0, 1.0, 1.0, -1.1174852513713567, 0.7805219884829433],
        [1.0, -2.0, 1.0, 1.0, -1.4319222143574686, 0.8216956697198521],
        [1.0, -2.0, 1.0, 1.0, -1.132618204157802, 0.9116810554754299],
        [1.0, -2.0, 1.0, 1.0, -1.560138940294104, 0.9344134406997735],
    ],
    "cheby1_8_high": [
        [0.028644503167599464, -0.05728900633519893, 0.028644503167599464, 1.0, 0.7436934476328694, 0.29559649904033336],
        [1.0, -2.0, 1.0, 1.0, -0.21592209789529263, 0.5959012584608236],
        [1.0, -2.0, 1.0, 1.0, -0.8553586521428111, 0.8126867993027922],
        [1.0, -2.0, 1.0, 1.0, -1.1392993192306604, 0.9446652958529225],
    ],
    "ellip8_0.05": [
        [0.00011310822400827776, -0.00014113959416038092, 0.00011310822400827776, 1.0, -1.8826448733040233, 0.8875241806574087],
        [1.0, -1.8779404709422802, 0.9999999999999999, 1.0, -1.9062858822489281, 0.9188027269126893],
        [1.0, -1.9370337005587996, 0.9999999999999998, 1.0, -1.9354464620705287, 0.9563453527455589],
        [1.0, -1.9505006616014862, 1.0, 1.0, -1.9610856966895565, 0.9867372934049468],
    ],
    "butter8_0.01": [
        [3.4219614165936484e-15, 6.843922833187297e-15, 3.4219614165936484e-15, 1.0, -1.939269633591658, 0.9402270185020654],
        [1.0, 2.0, 1.0, 1.0, -1.9481335385151675, 0.9490952993868512],
        [1.0, 2.0, 1.0, 1.0, -1.9647269019487286, 0.9656968546857874],
        [1.0, 2.0, 1.0, 1.0, -1.9868379069766875, 0.987818775546285],
    ],
    "butter2_0.001": [
        [2.461930046414063e-06, 4.923860092828126e-06, 2.461930046414063e-06, 1.0, -1.995557124345789, 0.9955669720659747],
    ],
    "butter12_0.002": [
        [9.023244006543289e-31, 1.8046488013086577e-30, 9.023244006543289e-31, 1.0, -1.98757911466523, 0.9876183485497565],
        [1.0, 2.0, 1.0, 1.0, -1.9884180173746582, 0.9884572678187328],
        [1.0, 2.0, 1.0, 1.0, -1.9900406600592244, 0.9900799425335086],
        [1.0, 2.0, 1.0, 1.0, -1.9923399495145508, 0.9923792773757364],
        [1.0, 2.0, 1.0, 1.0, -1.9951632412838627, 0.9952026248755107],
        [1.0, 2.0, 1.0, 1.0, -1.9983216684229461, 0.9983611143604724],
    ],
}.items()}

# held to K times the sequential float64 error; the last one, which float64
# handles badly whatever the method, to the project's 1e-9
BOUNDED = ["butter8_0.2", "butter6_band", "cheby1_8_high", "ellip8_0.05", "butter8_0.01",
           "butter2_0.001"]
ILL = "butter12_0.002"
K_BOUND = 8.0
FLOOR = 8.0 * 2.0 ** -53


def seq(sos, x, dt=LD, zi=None):
    """The cascade, section by section and sample by sample, on the rows of x
    (rows, n) in the type dt: (y, zf) with zf (rows, S, 2). The rows run side
    by side as vectors; the order of a row's operations is the recurrence's."""
    x = np.atleast_2d(np.asarray(x)).astype(dt)
    sos = np.asarray(sos).astype(dt)
    rows, n = x.shape
    S = len(sos)
    z = np.zeros((rows, S, 2), dt) if zi is None else np.asarray(zi).astype(dt).copy()
    y = x
    for s in range(S):
        b0, b1, b2, _, a1, a2 = sos[s]
        z0, z1 = z[:, s, 0].copy(), z[:, s, 1].copy()
        cols = np.ascontiguousarray(y.T)
        out = np.empty_like(cols)
        for i in range(n):
            xi = cols[i]
            yi = b0 * xi + z0
            z0 = b1 * xi - a1 * yi + z1
            z1 = b2 * xi - a2 * yi
            out[i] = yi
        y = np.ascontiguousarray(out.T)
        z[:, s, 0], z[:, s, 1] = z0, z1
    return y, z


def sosfilt_zi(sos):
    """scipy.signal.sosfilt_zi by its written formula, in long double."""
    zi = np.zeros((len(sos), 2), LD)
    scale = LD(1)
    for s, (b0, b1, b2, _, a1, a2) in enumerate(np.asarray(sos).astype(LD)):
        g = (b0 + b1 + b2) / (1 + a1 + a2)
        z1 = b2 - a2 * g
        zi[s] = scale * (b1 - a1 * g + z1), scale * z1
        scale = scale * g
    return zi


def padlen(sos):
    sos = np.asarray(sos)
    return 3 * (2 * len(sos) + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum())))


def odd_ext(x, pad):
    x = np.atleast_2d(x)
    return np.concatenate([2 * x[:, :1] - x[:, pad:0:-1], x, 2 * x[:, -1:] - x[:, -2:-pad - 2:-1]],
                          axis=1)


def sosfiltfilt(sos, x, pad=None, dt=LD):
    """scipy.signal.sosfiltfilt's composition (padtype="odd") in the type dt."""
    x = np.atleast_2d(np.asarray(x)).astype(dt)
    pad = padlen(sos) if pad is None else pad
    zi = sosfilt_zi(sos).astype(dt)
    ext = odd_ext(x, pad) if pad else x
    y, _ = seq(sos, ext, dt, zi[None] * ext[:, :1, None])
    y, _ = seq(sos, y[:, ::-1], dt, zi[None] * y[:, -1:, None])
    y = y[:, ::-1]
    return y[:, pad:y.shape[1] - pad] if pad else y


def err(a, ref):
    """max |a - ref| / max |ref| per row, the worst row."""
    a = np.atleast_2d(a).astype(LD)
    ref = np.atleast_2d(ref).astype(LD)
    return float(np.max(np.max(np.abs(a - ref), axis=1) / np.max(np.abs(ref), axis=1)))


# ---- the numpy model of the decomposition (float64, tables from long double)
def _chunk_run(sec, X, z0, z1):
    b0, b1, b2, _, a1, a2 = sec
    Y = np.empty_like(X)
    z0, z1 = z0.copy(), z1.copy()
    for i in range(X.shape[1]):
        xi = X[:, i]
        yi = b0 * xi + z0
        z0 = b1 * xi - a1 * yi + z1
        z1 = b2 * xi - a2 * yi
        Y[:, i] = yi
    return Y, z0, z1


def _zir(sec, steps):
    """c[i][j]: output i for unit state j; M: the state map over `steps`."""
    c = np.zeros((steps, 2))
    M = np.zeros((2, 2))
    for j in range(2):
        Y, z0, z1 = _chunk_run(sec.astype(LD), np.zeros((1, steps), LD),
                               np.array([1.0 if j == 0 else 0.0], LD),
                               np.array([1.0 if j == 1 else 0.0], LD))
        c[:, j] = Y[0].astype(float)
        M[:, j] = float(z0[0]), float(z1[0])
    return c, M


def _tile(sos, tabs, x, init):
    T = len(x) // E
    y = x.reshape(T, E).copy()
    fin = np.zeros_like(init)
    for s, sec in enumerate(sos):
        c, M = tabs[s]
        Y, f0, f1 = _chunk_run(sec, y, np.zeros(T), np.zeros(T))
        st = np.zeros((T + 1, 2))
        st[0] = init[s]
        for t in range(T):
            st[t + 1] = M @ st[t] + np.array([f0[t], f1[t]])
        y = Y + st[:T, 0:1] * c[None, :, 0] + st[:T, 1:2] * c[None, :, 1]
        fin[s] = st[T]
    return y.reshape(-1), fin


def model(sos, x):
    """One row of a whole number of tiles through the three passes."""
    sos = np.asarray(sos, dtype=np.float64)
    S = len(sos)
    nt = len(x) // TILE
    assert nt * TILE == len(x)
    tabs = [_zir(sec, E) for sec in sos]
    Phi = np.zeros((2 * S, 2 * S))
    for j in range(2 * S):
        e = np.zeros(2 * S, LD)
        e[j] = 1
        _, f = seq(sos, np.zeros((1, TILE)), LD, e.reshape(1, S, 2))
        Phi[:, j] = f.reshape(-1).astype(float)
    zero = np.zeros((S, 2))
    g = [_tile(sos, tabs, x[k * TILE:(k + 1) * TILE], zero)[1].reshape(-1) for k in range(nt)]
    st = np.zeros(2 * S)
    out = []
    for k in range(nt):
        out.append(_tile(sos, tabs, x[k * TILE:(k + 1) * TILE], st.reshape(S, 2))[0])
        st = Phi @ st + g[k]
    return np.concatenate(out)
