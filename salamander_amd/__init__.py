"""MI355X-native KL-NMF update engine behind Salamander's ``KLNMF`` / ``MvNMF`` API.

``import salamander_amd as sal; sal.models.KLNMF(n_signatures=50).fit(adata)`` is a
drop-in for the reference's fit path.  Importing the package needs
no GPU; every compute entry point raises :class:`EngineUnavailable` when the HIP
extension or a gfx950 device is missing -- there is no CPU fallback.
"""

from . import models
from ._lib import EngineUnavailable
from .anndata_compat import AnnData, MuData
from .assign import AssignResult, assign_signatures
from .change import ChangeResult, exposure_change_test
from .covariance import CovarianceResult, exposure_covariance
from .engine import Engine
from .gof import GofResult, draw_model_counts, goodness_of_fit
from .intervals import IntervalResult, ProfileResult, exposure_intervals, profile_likelihood
from .nb import (DispersionResult, DispersionTestResult, NBAssignResult, NBGofResult, NBPresenceResult, NBRefitResult, dispersion_test,
                 draw_nb_counts, estimate_dispersion, nb_assign_signatures, nb_goodness_of_fit, nb_refit_exposures, nb_signature_presence_test)
from .power import PowerResult, signature_power
from .presence import PresenceResult, signature_presence_test
from .refit import RefitResult, refit_exposures
from .resample import resample_counts
from .sigchange import SignatureChangeResult, signature_change_test
from .split import split_counts
from .stability import signature_stability

__version__ = "0.1.0"
__all__ = ["models", "Engine", "AnnData", "MuData", "EngineUnavailable", "resample_counts", "signature_stability", "refit_exposures", "RefitResult", "assign_signatures",
           "AssignResult", "split_counts", "goodness_of_fit", "draw_model_counts", "GofResult", "signature_presence_test",
           "PresenceResult", "signature_power", "PowerResult", "profile_likelihood", "ProfileResult", "exposure_intervals", "IntervalResult",
           "exposure_covariance", "CovarianceResult", "exposure_change_test", "ChangeResult", "signature_change_test",
           "SignatureChangeResult", "nb_refit_exposures", "NBRefitResult", "estimate_dispersion", "DispersionResult",
           "draw_nb_counts", "nb_goodness_of_fit", "NBGofResult", "dispersion_test", "DispersionTestResult",
           "nb_assign_signatures", "NBAssignResult", "nb_signature_presence_test", "NBPresenceResult"]
