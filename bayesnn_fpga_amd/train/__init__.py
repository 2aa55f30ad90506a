from .calibration import EnsembleTemperatureScaling, EnsembleWeights, TemperatureScaling  # noqa: F401
from .evaluate import MultiExitAccuracy, evaluate, evaluate_exits  # noqa: F401
from .exit_policy import ExitPolicyAnalysis, policy_macs, policy_metrics, reference_costs  # noqa: F401
from .ranking import RankingAnalysis, rank_metrics, risk_at_coverage, threshold_at_coverage  # noqa: F401
from .reliability import ReliabilityAnalysis  # noqa: F401
from .results_analyzer import FullAnalysis  # noqa: F401
from .uncertainty import UncertaintyAnalysis, average_predictive_entropy  # noqa: F401
