from .beam import Beam  # noqa: F401
from .parameter_beam import ParameterBeam  # noqa: F401
from .particle_beam import ParticleBeam  # noqa: F401
from .species import Species  # noqa: F401
from .slices import BeamSlices  # noqa: F401
from .turns import TurnByTurn  # noqa: F401
from .optics import ClosedOrbit, OneTurnMap, RadiationIntegrals, RingOptics, RingSensitivity, eigen_tunes, propagate_twiss, twiss_from_matrix  # noqa: F401
