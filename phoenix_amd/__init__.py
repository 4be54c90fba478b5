"""phoenix_amd -- MI355X-native NeuralODE integration engine for PHOENIX's ODENet.

Drop-in for the reference's hot path only:  `from phoenix_amd import odeint_adjoint as odeint`
replaces `from torchdiffeq import odeint_adjoint as odeint` (train_insilico.py:15-18)."""
from .odeint import SOLVERS, odeint, odeint_adjoint, odeint_calls, odeint_per_sample  # noqa: F401
from .odenet import ODENet  # noqa: F401
from .engine import check_pending_status, set_status_mode  # noqa: F401
from .training import get_true_val_set_r2, my_r_squared, training_step, validation  # noqa: F401
from .graphs import GraphedStep  # noqa: F401
from .data import DataHandler, readcsv, writecsv  # noqa: F401
from .prior import PriorMatrix, prior_targets, read_prior_matrix  # noqa: F401
from .analysis import (Edges, EpistasisPerPair, EpistasisRecovery, EpistasisRecoveryScores,  # noqa: F401
                       JacobianRecovery, KnockoutEffects, KnockoutPairs, KnockoutPerGene, KnockoutRecovery, KnockoutRecoveryScores, Neighbors, NetworkScore, Pathways,
                       PermutationTest, consolidate_gene_scores, effects_at, effects_edges, effects_matrix,
                       effects_neighbors, epistasis_recovery, epistasis_recovery_scores, gene_influence_matrix,
                       gene_influence_scores, jacobian_matrix,
                       jacobian_recovery, knockout_effects, knockout_pairs, knockout_recovery, knockout_recovery_scores,
                       network_score,
                       Propagation, effects_apply, network_propagation, propagation_reference,
                       pathway_permutation_test, read_network, read_pathways, recovery_scores, write_link_list,
                       write_permutation_table, SteadyStateRecovery, steady_state_recovery, steady_state_recovery_scores)
from .simulator import (HillBlocks, HillJacobian, HillPattern, HillSystem, block_substitution,  # noqa: F401
                        generate_dataset, jacobian_reference, knockouts_reference, rates_reference)
from .steady import (KnockoutSteadyStates, SteadyAdjoint, SteadyResponse, SteadyStates,  # noqa: F401
                     knockout_steady_states,
                     last_backward_info, reduced_jacobian, steady_states, steady_states_adjoint_reference,
                     steady_state_response, steady_state_response_reference, steady_states_reference)

__version__ = "0.1.0"
