"""bocf_amd: MI355X-native GP-posterior + composite-acquisition hot path of BOCF behind the
reference's multi_outputGP / AcquisitionBase plug-in surface.  See DESIGN.md."""
from . import _ffi, kern, utility_program  # noqa: F401
from .acquisition_optimizer import AcquisitionOptimizer, Design_space  # noqa: F401
from .acquisitions import EI, PI, UCB, AcquisitionBase, LogEI, maEI, maLogEI, maPI, maUCB, uCVaR, uLogEI, uEI_constrained, uEI_joint, uEI_noiseless, uEI_pending, uKG, uPI, uUCB  # noqa: F401
from .constraints import OutputConstraints  # noqa: F401
from .cbo import CBO, CompositeGreedyBatch, CompositeJointBatch, CompositePathwiseThompsonBatch, CompositeThompsonBatch, Sequential  # noqa: F401
from .multi_outputGP import multi_outputGP  # noqa: F401
from .objective import MultiObjective  # noqa: F401
from .recommend import current_marginal_argmaxes  # noqa: F401
from .utility import ExpectationUtility, ParameterDistribution, Utility  # noqa: F401
from .utility_program import TraceError  # noqa: F401

__version__ = "0.1.0"
