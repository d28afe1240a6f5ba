"""The periodic dv/dr correction of coeval boxes on the MI355X (csrc/hip/dvdr_periodic_kernels.hip,
csrc/host/dvdr_periodic_driver.c, grid_api.dvdr_periodic, rsds.include_dvdr_in_tau21, drivers.Coeval),
against the fp64 restatement of tests/dvdr_periodic_reference.py.

Tolerance.  The reference computes the gradient with scipy.fft on float32 input, in single precision.  Per
test, on the test's own input: delta = 4 max|g_f32 - g_f64| with g_f32 the reference's expression on the
float32 velocities and g_f64 the restatement, and never below 4 eps32 max|g_f64| (the factor 4 covers another
butterfly order and the fp32 multiplication by k).  Taylor form: |out - want| <= |want| (delta / (H (1 -
max_dvdr)) + 2 eps32): d ln(out) / dg = 1 / (H |1 + g/H|) <= 1 / (H (1 - max_dvdr)) under the clip, and two
float32 roundings.  tau form: out lies between the fp64 formula at g - delta and at g + delta, widened by
2 eps32 relative; its inputs are scaled to max|g| / H = 0.5 and the test asserts |1 + g/H| >= 0.25 in every
cell, so the factor is monotonic between the two.  tau_21 >= 1e-4 (apart from the cells set below the
1e-10 threshold) keeps the cancellation in 1 - exp(-tau), 2^-53 / tau relative, far below eps32.  No cell
is left out of any comparison.  Every comparison prints its largest error / tolerance."""

import importlib

import numpy as np
import pytest

import dvdr_periodic_reference as PR
import lightcone_reference as LR
from test_gpu_run_coeval import DATA

pytestmark = pytest.mark.gpu
D = importlib.import_module("21cmfast_amd.drivers")
api = importlib.import_module("21cmfast_amd.grid_api")
rsds = importlib.import_module("21cmfast_amd.rsds")

EPS = float(np.finfo(np.float32).eps)
MAX_DVDR = 0.2
FFT_N = [8, 16, 64, 128, 512, 1024]
DIRECT_N = [2, 3, 5, 12, 35, 50, 96, 200]
N_COLS = [1, 7, 130, 33 * 33]


def hubble_table(n):
    """H(z) [1/s] per slice, falling by a few per cent along the line."""
    return 2.2e-18 * (1.0 + 0.05 * np.linspace(0.0, 1.0, n))


def delta_for(vel32, dx, g64):
    """4 x the error of the reference's single-precision gradient on this input, floored at 4 eps32 max|g|."""
    from scipy import fft

    n = vel32.shape[-1]
    k = fft.rfftfreq(n, dx) * 2.0 * np.pi
    g32 = fft.irfft(1j * k * fft.rfft(vel32, axis=-1), n=n, axis=-1)  # rsds.py:64-70 along the last axis
    return max(4.0 * float(np.abs(g32 - g64).max()), 4.0 * EPS * float(np.abs(g64).max()))


def check_taylor(got, bt, g64, H, delta, what, want=None):
    want = PR.taylor_form(bt, g64, H, MAX_DVDR) if want is None else want
    tol = np.abs(want) * (delta / (H * (1.0 - MAX_DVDR)) + 2.0 * EPS)
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: taylor worst error / tolerance = {ratio:.3f}")
    assert (err <= tol).all(), f"{what}: worst {ratio} x tolerance"
    return ratio


def check_tau(got, bt, tau, g64, H, delta, what):
    assert (np.abs(1.0 + g64 / H) >= 0.25).all()
    a = np.asarray(bt, np.float64) * PR.tau_factor(tau, g64 - delta, H)
    b = np.asarray(bt, np.float64) * PR.tau_factor(tau, g64 + delta, H)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    lo, hi = lo - 2.0 * EPS * np.abs(lo), hi + 2.0 * EPS * np.abs(hi)
    got = np.asarray(got, np.float64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    ratio = float((np.abs(got - mid) / np.maximum(half, 1e-300)).max())
    print(f"{what}: tau worst error / tolerance = {ratio:.3f}")
    assert ((got >= lo) & (got <= hi)).all(), f"{what}: worst {ratio} x tolerance"
    return ratio


def make_case(n_cols, n, use_ts, seed, dx=1.5):
    """Seeded (bt, vel, tau, H, g64): Taylor gradients of order 0.3 H (the clip engages in part of the cells),
    tau-form gradients normalised to max|g| / H = 0.5 by the fp64 gradient of the draw."""
    rng = np.random.default_rng(seed)
    H = hubble_table(n)
    raw = rng.standard_normal((n_cols, n))
    g_raw = PR.gradient_rfft(raw, dx)
    if n == 2:  # the gradient vanishes identically: any velocity will do
        vel = (raw * 0.3 * H * dx).astype(np.float32)
    elif use_ts:
        vel = (raw * 0.5 / np.abs(g_raw / H).max()).astype(np.float32)
    else:
        vel = (raw * 0.3 * H.mean() / g_raw.std()).astype(np.float32)
    bt = (rng.standard_normal((n_cols, n)) * 20.0).astype(np.float32)
    tau = None
    if use_ts:
        tau = (np.abs(rng.standard_normal((n_cols, n))) * 0.05 + 1e-4).astype(np.float32)
        tau[:, 0] = 1e-11  # below the 1e-10 threshold
        if n > 2:
            tau[:, 2] = 0.0
    return bt, vel, tau, H, PR.gradient_rfft(vel, dx)


def run(bt, vel, H, dx, tau=None, method="auto", device=True, out=None):
    import torch

    if not device:
        return api.dvdr_periodic(bt, vel, H, dx, MAX_DVDR, tau_21=tau, method=method, out=out)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()  # noqa: E731
    return api.dvdr_periodic(dev(bt), dev(vel), H, dx, MAX_DVDR, tau_21=dev(tau), method=method).cpu().numpy()


@pytest.mark.parametrize("use_ts", [False, True])
@pytest.mark.parametrize("n", FFT_N + DIRECT_N)
def test_kernel_matches_restatement(gpu_lib, n, use_ts):
    dx = 1.5
    for n_cols in N_COLS:
        bt, vel, tau, H, g64 = make_case(n_cols, n, use_ts, seed=1000 * n + n_cols, dx=dx)
        delta = delta_for(vel, dx, g64)
        got = run(bt, vel, H, dx, tau)
        what = f"n={n} n_cols={n_cols} {'fft' if n in FFT_N else 'direct'}"
        if use_ts:
            check_tau(got, bt, tau, g64, H, delta, what)
            small = tau < 1e-10
            assert small.any()
            np.testing.assert_array_equal(got[small], bt[small])  # bit-identical below the threshold
        else:
            if n > 2 and n_cols >= 130:
                assert np.mean(np.abs(g64) > MAX_DVDR * H) > 0.1  # the clip does engage
            check_taylor(got, bt, g64, H, delta, what)


@pytest.mark.parametrize("use_ts", [False, True])
@pytest.mark.parametrize("n,method", [(32, "auto"), (256, "auto"), (1536, "auto"), (1024, "direct")])
def test_remaining_instantiations_and_the_longest_line(gpu_lib, n, method, use_ts):
    """The two transform shapes the list above leaves out, the longest line of the direct path and the
    longest line the direct path can be forced onto; an odd count of lines."""
    dx = 1.5
    bt, vel, tau, H, g64 = make_case(131, n, use_ts, seed=31 * n, dx=dx)
    delta = delta_for(vel, dx, g64)
    got = run(bt, vel, H, dx, tau, method=method)
    if use_ts:
        check_tau(got, bt, tau, g64, H, delta, f"n={n} {method}")
    else:
        check_taylor(got, bt, g64, H, delta, f"n={n} {method}")


@pytest.mark.parametrize("n", [8, 64, 512])
def test_the_two_paths_agree(gpu_lib, n):
    dx = 1.5
    bt, vel, _, H, g64 = make_case(130, n, False, seed=77 + n, dx=dx)
    delta = delta_for(vel, dx, g64)
    a, b = run(bt, vel, H, dx, method="fft"), run(bt, vel, H, dx, method="direct")
    want = np.abs(PR.taylor_form(bt, g64, H, MAX_DVDR))
    err = np.abs(a.astype(np.float64) - b)
    print(f"n={n}: fft vs direct worst difference / (2 delta / H) = {float((err / (want * 2 * delta / H)).max()):.3f}")
    assert (err <= want * 2.0 * delta / H).all()
    np.testing.assert_array_equal(run(bt, vel, H, dx, method="auto"), a)


def test_methods_that_do_not_fit_are_value_errors(gpu_lib):
    import ctypes as C

    S = importlib.import_module("21cmfast_amd.structs")
    for n, method in ((50, "fft"), (1537, "direct"), (1537, "auto"), (2048, "fft")):
        a = np.ones((3, n), np.float32)
        with pytest.raises(ValueError):
            api.dvdr_periodic(a, a, 2.2e-18, 1.5, MAX_DVDR, method=method)
    with pytest.raises(ValueError):
        api.dvdr_periodic(np.ones((3, 8), np.float32), np.ones((3, 8), np.float32), 2.2e-18, 1.5, MAX_DVDR,
                          method="rocfft")
    # the library makes the same checks itself and launches nothing
    gpu_lib.c21cm_dvdr_periodic_grids.restype = C.c_int
    gpu_lib.c21cm_last_error.restype = C.c_char_p

    def call(n=8, tau=None, null_vel=False, **kw):
        hub = np.full(n, 2.2e-18)
        spec = dict(n_cols=3, n_slices=n, dx=1.5, max_dvdr=0.2, use_ts_fluct=0, method=0,
                    hubble=hub.ctypes.data_as(S.c_double_p))
        spec.update(kw)
        a, out = np.ones((3, n), np.float32), np.full((3, n), 7.0, np.float32)
        st = gpu_lib.c21cm_dvdr_periodic_grids(C.byref(S.DvdrPeriodicSpec(**spec)), C.c_void_p(a.ctypes.data),
                                               None if null_vel else C.c_void_p(a.ctypes.data), tau,
                                               C.c_void_p(out.ctypes.data), None)
        assert st == 0 or (out == 7.0).all()
        return st

    assert call() == 0
    bad = (dict(n=50, method=1), dict(n=1537, method=2), dict(n=1537), dict(n_slices=1), dict(method=3),
           dict(dx=0.0), dict(dx=float("nan")), dict(max_dvdr=-1.0), dict(use_ts_fluct=1), dict(null_vel=True),
           dict(n_cols=-1), dict(hubble=None))
    for kw in bad:
        assert call(**kw) == 3, kw  # C21CM_VALUE_ERROR
        assert b"periodic dvdr" in gpu_lib.c21cm_last_error()
    assert call(n_cols=0) == 0


@pytest.mark.parametrize("method,n", [("fft", 8), ("fft", 64), ("direct", 8), ("direct", 64), ("direct", 50),
                                      ("direct", 35)])
@pytest.mark.parametrize("use_ts", [False, True])
def test_constant_and_nyquist_lines_leave_the_box_unchanged(gpu_lib, method, n, use_ts):
    rng = np.random.default_rng(n)
    n_cols, dx, H = 37, 1.5, hubble_table(n)
    bt = (rng.standard_normal((n_cols, n)) * 20.0).astype(np.float32)
    tau = (np.abs(rng.standard_normal((n_cols, n))) * 0.05 + 1e-4).astype(np.float32) if use_ts else None
    amp = (rng.standard_normal((n_cols, 1)) * 1e-17).astype(np.float32)  # Mpc/s, as a velocity
    lines = [np.broadcast_to(amp, (n_cols, n))]
    if n % 2 == 0:
        lines.append(amp * ((-1.0) ** np.arange(n)).astype(np.float32))
    for vel in lines:
        got = run(bt, np.ascontiguousarray(vel, np.float32), H, dx, tau, method=method)
        assert (np.abs(got.astype(np.float64) - bt) <= np.spacing(np.abs(bt))).all()  # 1 ulp


@pytest.mark.parametrize("method,n,mode", [("fft", 64, 16), ("direct", 64, 16), ("direct", 50, 12), ("fft", 512, 100)])
def test_single_sine_mode(gpu_lib, method, n, mode):
    dx, H = 1.5, hubble_table(n)
    k = 2.0 * np.pi * mode / (n * dx)
    x = dx * np.arange(n)
    phase = np.linspace(0.0, 2.0 * np.pi, 9, endpoint=False)[:, None]
    amp = 0.15 * H.min() / k  # inside the clip
    vel = (amp * np.sin(k * x + phase)).astype(np.float32)
    analytic = amp * k * np.cos(k * x + phase)
    bt = np.full(vel.shape, 25.0, np.float32)
    delta = delta_for(vel, dx, PR.gradient_rfft(vel, dx))
    got = run(bt, vel, H, dx, method=method)
    check_taylor(got, bt, analytic, H, delta, f"sine n={n} {method}")


@pytest.mark.parametrize("method,n", [("fft", 64), ("direct", 50)])
def test_clip_bounds_every_output(gpu_lib, method, n):
    rng = np.random.default_rng(3)
    dx, H = 1.5, hubble_table(n)
    raw = rng.standard_normal((130, n))
    vel = (raw * 0.5 * H.mean() / PR.gradient_rfft(raw, dx).std()).astype(np.float32)
    g64 = PR.gradient_rfft(vel, dx)
    assert np.mean(np.abs(g64) > MAX_DVDR * H) > 1.0 / 3.0
    bt = (np.abs(rng.standard_normal((130, n))) * 20.0 + 1.0).astype(np.float32)
    got = run(bt, vel, H, dx, method=method).astype(np.float64)
    lo, hi = bt / (1.0 + MAX_DVDR), bt / (1.0 - MAX_DVDR)
    assert (got >= lo * (1.0 - 2.0 * EPS)).all() and (got <= hi * (1.0 + 2.0 * EPS)).all()
    check_taylor(got, bt, g64, H, delta_for(vel, dx, g64), f"clipped n={n} {method}")


@pytest.mark.parametrize("n,use_ts", [(64, False), (64, True), (50, False), (50, True)])
def test_plumbing(gpu_lib, n, use_ts):
    import torch

    dx = 1.5
    bt, vel, tau, H, _ = make_case(131, n, use_ts, seed=9 + n, dx=dx)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()  # noqa: E731
    d_bt, d_vel, d_tau = dev(bt), dev(vel), dev(tau)
    first = api.dvdr_periodic(d_bt, d_vel, H, dx, MAX_DVDR, tau_21=d_tau)
    assert first.is_cuda and first.data_ptr() != d_bt.data_ptr()
    got = first.cpu().numpy()
    # the inputs are untouched, two calls give the same bits
    np.testing.assert_array_equal(d_bt.cpu().numpy(), bt)
    np.testing.assert_array_equal(d_vel.cpu().numpy(), vel)
    if use_ts:
        np.testing.assert_array_equal(d_tau.cpu().numpy(), tau)
    np.testing.assert_array_equal(api.dvdr_periodic(d_bt, d_vel, H, dx, MAX_DVDR, tau_21=d_tau).cpu().numpy(), got)
    # numpy arrays in: numpy out, the same bits, the inputs untouched
    h_bt, h_vel, h_tau = bt.copy(), vel.copy(), None if tau is None else tau.copy()
    host = api.dvdr_periodic(h_bt, h_vel, H, dx, MAX_DVDR, tau_21=h_tau)
    assert isinstance(host, np.ndarray) and host is not h_bt
    np.testing.assert_array_equal(host, got)
    np.testing.assert_array_equal(h_bt, bt)
    np.testing.assert_array_equal(h_vel, vel)
    # out aliasing brightness_temp, on the device and on the host
    assert api.dvdr_periodic(d_bt, d_vel, H, dx, MAX_DVDR, tau_21=d_tau, out=d_bt) is d_bt
    np.testing.assert_array_equal(d_bt.cpu().numpy(), got)
    api.dvdr_periodic(h_bt, h_vel, H, dx, MAX_DVDR, tau_21=h_tau, out=h_bt)
    np.testing.assert_array_equal(h_bt, got)
    np.testing.assert_array_equal(h_vel, vel)
    # a device view that starts off a 16-byte boundary takes the scalar accesses: the same bits
    pad = lambda a: None if a is None else torch.cat([torch.zeros(1, device="cuda"), dev(a).flatten()])[1:].view(a.shape)  # noqa: E731
    off = api.dvdr_periodic(pad(bt), pad(vel), H, dx, MAX_DVDR, tau_21=pad(tau))
    np.testing.assert_array_equal(off.cpu().numpy(), got)
    # a per-slice H(z) is honoured (the comparisons above use one): a scalar H(z_0) changes every slice but the first
    flat = api.dvdr_periodic(dev(bt), d_vel, float(H[0]), dx, MAX_DVDR, tau_21=d_tau).cpu().numpy()
    assert (flat != got).any()
    np.testing.assert_array_equal(flat[:, 0], got[:, 0])


# ---- the public interface -----------------------------------------------------------------------------
def box_inputs(n, **kw):
    return D.Inputs(random_seed=4, HII_DIM=n, DIM=2 * n, BOX_LEN=2.0 * n, N_THREADS=2, SOURCE_MODEL=1,
                    HII_FILTER=0, **kw)


def hubble_of(inputs, z):
    cosmo = D.FlatCosmology(inputs.cosmo_params.hlittle, inputs.cosmo_params.OMm)
    return float(cosmo.H0_cgs * cosmo.efunc(z))


def synthetic_box(n, z, use_ts, seed):
    inputs = box_inputs(n, USE_TS_FLUCT=True) if use_ts else box_inputs(n)
    H = hubble_of(inputs, z)
    bt, vel, tau, _, _ = make_case(n * n, n, use_ts, seed=seed, dx=2.0)
    vel = (vel.astype(np.float64) * H / hubble_table(n).mean()).astype(np.float32)  # gradients of order H(z)
    if use_ts:  # max|g| / H = 0.5 again, after the rounding of the velocities
        vel = (vel * (0.5 * H / np.abs(PR.gradient_rfft(vel, 2.0)).max())).astype(np.float32)
    shape = (n, n, n)
    return inputs, H, bt.reshape(shape), vel.reshape(shape), None if tau is None else tau.reshape(shape)


def test_include_dvdr_periodic_and_not(gpu_lib):
    import torch

    z = 9.0
    inputs, H, bt, vel, _ = synthetic_box(32, z, False, seed=5)
    g64 = PR.gradient_rfft(vel, 2.0)
    got = rsds.include_dvdr_in_tau21(bt, vel, z, inputs, periodic=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == bt.shape
    check_taylor(got, bt, g64, np.full(32, H), delta_for(vel, 2.0, g64), "rsds 32^3")
    # 2-D input: the same numbers; a redshift per slice: the same again; torch in, torch out, the same bits
    flat = rsds.include_dvdr_in_tau21(bt.reshape(-1, 32), vel.reshape(-1, 32), z, inputs, periodic=True)
    np.testing.assert_array_equal(flat.reshape(bt.shape), got)
    np.testing.assert_array_equal(rsds.include_dvdr_in_tau21(bt, vel, np.full(32, z), inputs, periodic=True), got)
    d_bt, d_vel = torch.from_numpy(bt).cuda(), torch.from_numpy(vel).cuda()
    dev = rsds.include_dvdr_in_tau21(d_bt, d_vel, z, inputs, periodic=True)
    assert dev.is_cuda and dev.data_ptr() != d_bt.data_ptr()
    np.testing.assert_array_equal(dev.cpu().numpy(), got)
    np.testing.assert_array_equal(d_bt.cpu().numpy(), bt)
    # periodic = False: the lightcone kernel on a copy, compared as the lightcone tests compare it
    before = bt.copy()
    open_ = rsds.include_dvdr_in_tau21(bt, vel, z, inputs, periodic=False)
    want = LR.include_dvdr_in_tau21(bt, vel, np.full(32, H), 2.0, MAX_DVDR)
    np.testing.assert_allclose(open_, want, rtol=1e-6, atol=1e-30)
    np.testing.assert_array_equal(bt, before)
    dev_open = rsds.include_dvdr_in_tau21(d_bt, d_vel, z, inputs, periodic=False)
    np.testing.assert_array_equal(dev_open.cpu().numpy(), open_)
    np.testing.assert_array_equal(d_bt.cpu().numpy(), bt)
    assert (open_ != got).any()


def test_coeval_methods_on_a_run_coeval_snapshot(gpu_lib, monkeypatch):
    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    inputs = box_inputs(32, KEEP_3D_VELOCITIES=True)
    result = D.run_coeval(inputs, [18.0], data_path=DATA, device="cuda", lib=gpu_lib)
    coeval = D.Coeval.from_result(result, 18.0, inputs)
    bt = coeval.brightness_temp
    H = hubble_of(inputs, 18.0)
    for axis in ("z", "x"):
        vel = getattr(coeval, "velocity_" + axis)
        tb = coeval.include_dvdr_in_tau21(axis=axis)
        assert tb.is_cuda and tuple(tb.shape) == tuple(bt.shape) == (32, 32, 32)
        v32 = vel.cpu().numpy()
        g64 = PR.gradient_rfft(v32, 2.0)
        check_taylor(tb.cpu().numpy(), bt.cpu().numpy(), g64, np.full(32, H), delta_for(v32, 2.0, g64),
                     f"run_coeval axis={axis}")
        shifted = coeval.apply_rsds(axis=axis)
        both = coeval.apply_velocity_corrections(axis=axis)
        assert tuple(shifted.shape) == tuple(both.shape) == (32, 32, 32)
        want = rsds.apply_rsds(rsds.include_dvdr_in_tau21(bt, vel, 18.0, inputs, periodic=True), vel, 18.0, inputs,
                               periodic=True)
        np.testing.assert_array_equal(both.cpu().numpy(), want.cpu().numpy())
        np.testing.assert_array_equal(shifted.cpu().numpy(),
                                      rsds.apply_rsds(bt, vel, 18.0, inputs, periodic=True).cpu().numpy())
    assert (coeval.apply_rsds(field="density").cpu().numpy() != coeval.density.cpu().numpy()).any()


def test_coeval_tau_form_on_synthetic_arrays(gpu_lib):
    z = 9.0
    inputs, H, bt, vel, tau = synthetic_box(32, z, True, seed=6)
    fields = {"brightness_temp": bt, "velocity_z": vel, "tau_21": tau}
    coeval = D.Coeval(inputs, z, fields)
    g64 = PR.gradient_rfft(vel, 2.0)
    tb = coeval.include_dvdr_in_tau21()
    check_tau(tb, bt, tau, g64, np.full(32, H), delta_for(vel, 2.0, g64), "Coeval tau form")
    both = coeval.apply_velocity_corrections()
    np.testing.assert_array_equal(both, rsds.apply_rsds(tb, vel, z, inputs, periodic=True))
    fields.pop("tau_21")
    for call in (D.Coeval(inputs, z, fields).include_dvdr_in_tau21,
                 D.Coeval(inputs, z, fields).apply_velocity_corrections):
        with pytest.raises(ValueError, match=r'keep=\(\.\.\., "tau_21"\) to run_coeval'):
            call()


# ---- one shape of production size ---------------------------------------------------------------------
def test_production_shapes(gpu_lib):
    import torch

    z = 9.0
    inputs, H, bt, vel, _ = synthetic_box(128, z, False, seed=11)
    coeval = D.Coeval(inputs, z, {"brightness_temp": torch.from_numpy(bt).cuda(),
                                  "velocity_z": torch.from_numpy(vel).cuda()})
    g64 = PR.gradient_rfft(vel, 2.0)
    check_taylor(coeval.include_dvdr_in_tau21().cpu().numpy(), bt, g64, np.full(128, H),
                 delta_for(vel, 2.0, g64), "Coeval 128^3")
    for use_ts in (False, True):
        bt, vel, tau, Hs, g64 = make_case(4096, 512, use_ts, seed=12 + use_ts)
        got, delta = run(bt, vel, Hs, 1.5, tau), delta_for(vel, 1.5, g64)
        if use_ts:
            check_tau(got, bt, tau, g64, Hs, delta, "512 x 4096")
        else:
            check_taylor(got, bt, g64, Hs, delta, "512 x 4096")
