"""ScalarDiffusivity / VerticalScalarDiffusivity with Explicit or VerticallyImplicit time discretisation (Oceananigans.TurbulenceClosures,
re-exported by the reference; its users: test/turbulence_closures.jl:14-20, test/vertical_diffusion.jl,
validation/DCMIP2016_TC/dcmip2016_tc.jl:277-281).  Data only: csrc/bz_diffusivity.hip computes, include/breeze_hip.h states the reading."""
import numbers


class ExplicitTimeDiscretization:
    """ExplicitTimeDiscretization(): every flux of the closure enters the tendencies (the default)."""


class VerticallyImplicitTimeDiscretization:
    """VerticallyImplicitTimeDiscretization(): the vertical fluxes are advanced by implicit_step! after each RK update."""


def _coefficient(name, value):
    from .model import Field
    if isinstance(value, Field):
        if value.zface or any(l.__name__ != "Center" for l in value.loc):
            raise NotImplementedError(f"{name}: a field-valued coefficient is a (Center, Center, Center) field of the model's grid")
        return value
    if isinstance(value, (dict, tuple, list)):
        raise NotImplementedError(f"{name}: one diffusivity for every scalar is implemented (no per-tracer mapping)")
    if callable(value):
        raise NotImplementedError(f"{name}: a number or a centre Field is implemented (no function of x, y, z, t)")
    if isinstance(value, numbers.Real) and not isinstance(value, bool):
        if value < 0:
            raise ValueError(f"{name} must not be negative")
        return float(value)
    raise TypeError(f"{name}: a number or a centre Field, got {type(value).__name__}")


class ScalarDiffusivity:
    """ScalarDiffusivity(time_discretization = ExplicitTimeDiscretization(); ν = 0, κ = 0): isotropic viscosity ν and diffusivity κ
    (every scalar), each a number or a centre Field that the user may rewrite between steps (call update_state_(model) afterwards,
    as after set!)."""
    formulation = 0

    def __init__(self, time_discretization=None, ν=0.0, κ=0.0, nu=None, kappa=None):
        if isinstance(time_discretization, type):
            time_discretization = time_discretization()
        if time_discretization is None:
            time_discretization = ExplicitTimeDiscretization()
        if not isinstance(time_discretization, (ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization)):
            raise TypeError("the positional argument is ExplicitTimeDiscretization() or VerticallyImplicitTimeDiscretization()")
        self.time_discretization = time_discretization
        self.ν = _coefficient("ν", ν if nu is None else nu)
        self.κ = _coefficient("κ", κ if kappa is None else kappa)

    @property
    def vertically_implicit(self):
        return isinstance(self.time_discretization, VerticallyImplicitTimeDiscretization)


class VerticalScalarDiffusivity(ScalarDiffusivity):
    """VerticalScalarDiffusivity(time_discretization; ν = 0, κ = 0): only the z components of the fluxes exist."""
    formulation = 1


class HorizontalScalarDiffusivity:
    """Named so that asking for it says what is missing."""

    def __init__(self, *a, **kw):
        raise NotImplementedError("HorizontalScalarDiffusivity is not implemented (ScalarDiffusivity and VerticalScalarDiffusivity are)")


class DynamicSmagorinsky:
    """Named so that asking for it says what is missing."""

    def __init__(self, *a, **kw):
        raise NotImplementedError("DynamicSmagorinsky is not implemented (SmagorinskyLilly is)")


class AnisotropicMinimumDissipation:
    """Named so that asking for it says what is missing."""

    def __init__(self, *a, **kw):
        raise NotImplementedError("AnisotropicMinimumDissipation is not implemented (SmagorinskyLilly is)")
