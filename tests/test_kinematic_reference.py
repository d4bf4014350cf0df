"""Pins tests/kinematic_reference.py — the CPU restatement of AtmosphereModel(dynamics = PrescribedDynamics(...)) — before
tests/test_kinematic.py compares the device with it: the reference's own analytic advection test, the two properties the divergence
correction exists for, and conservation of tracer mass."""
import numpy as np

from kinematic_reference import KinematicReference, velocity_field

EPS = np.finfo(np.float64).eps


def test_gaussian_advection_meets_the_references_threshold(oracle):
    """test/kinematic_driver.jl:89-115: a Gaussian tracer carried upward by w0 = 10 for 50 steps of 1 s stays within 0.1 of the analytic
    profile.  (set!(model, c = ...) sets the tracer's density field, and that field is what the reference compares.)"""
    Lz, Nz, w0, z0, sigma = 4000.0, 64, 10.0, 1000.0, 100.0
    exact = lambda t: (lambda x, y, z: np.exp(-(z - z0 - w0 * t) ** 2 / (2 * sigma ** 2)) + 0 * x + 0 * y)
    k = KinematicReference(oracle, (4, 4, Nz), x=(0, 100), y=(0, 100), z=(0, Lz), potential_temperature=288.0, tracers=1)
    k.set(theta=300.0, qt=0.0, w=w0, rc0=exact(0.0))
    for _ in range(50):
        k.time_step(1.0)
    x, y, z = k.grid.nodes("ccc")
    err = np.abs(k.interior("rc0") - exact(50.0)(x, y, z)).max()
    print("gaussian advection: max error", err)
    assert err < 0.1


def divergent_case(oracle, correction):
    Lx, Ly, Lz = 2400.0, 1200.0, 3000.0
    zf = Lz * (np.arange(11) / 10.0) ** 1.3          # stretched
    k = KinematicReference(oracle, (24, 12, 10), x=(0, Lx), y=(0, Ly), z=zf, tracers=1, divergence_correction=correction)
    u, v, w = velocity_field(Lx, Ly, Lz)
    rho = k.m.ref.density[k.grid.Hz:k.grid.Hz + k.grid.Nz][:, None, None]
    k.set(theta=300.0, qt=0.0, u=u, v=v, w=w, rc0=rho * np.ones((10, 12, 24)))          # c = 1
    return k


def test_uniform_tracer_is_steady_with_the_correction(oracle):
    k = divergent_case(oracle, True)
    assert np.all(k.interior("c0") == 1.0)
    assert np.abs(k.div_rhoU()).max() > 1e-3          # the field is divergent
    G = k.compute_tendencies()["rc0"]
    bound = 64 * EPS * k.max_mass_flux() / k.min_spacing()
    print("c = 1 with correction: max|G|", np.abs(G).max(), "bound", bound)
    assert np.abs(G).max() <= bound


def test_uniform_tracer_feels_the_divergence_without_the_correction(oracle):
    k = divergent_case(oracle, False)
    G = k.compute_tendencies()["rc0"]
    D = k.div_rhoU()
    bound = 64 * EPS * k.max_mass_flux() / k.min_spacing()
    print("c = 1 without correction: max|G|", np.abs(G).max(), "max|D|", np.abs(D).max(), "bound", bound)
    assert abs(np.abs(G).max() - np.abs(D).max()) <= bound
    assert np.abs(G + D).max() <= bound          # cell by cell: G = -D for c = 1


def test_tracer_mass_is_conserved_without_the_correction(oracle):
    Lx, Ly, Lz = 2400.0, 1200.0, 3000.0
    k = KinematicReference(oracle, (24, 12, 10), x=(0, Lx), y=(0, Ly), z=(0, Lz), tracers=1)
    u, v, w = velocity_field(Lx, Ly, Lz)
    k.set(theta=300.0, qt=0.0, u=u, v=v, w=w,
          rc0=lambda x, y, z: 1.0 + 0.5 * np.sin(2 * np.pi * x / Lx) * np.cos(2 * np.pi * y / Ly) * np.exp(-z / 2e3))
    assert np.all(k.interior("w")[0] == 0.0) and np.all(k.interior("w")[-1] == 0.0)
    V = k.cell_volumes()
    before = np.sum(k.interior("rc0") * V)
    for _ in range(3):
        k.time_step(5.0)
    after = np.sum(k.interior("rc0") * V)
    print("tracer mass: relative change", abs(after - before) / before)
    assert np.abs(k.interior("rc0") - 1.0).max() > 0.01          # it moved
    assert abs(after - before) <= 1e-13 * before
