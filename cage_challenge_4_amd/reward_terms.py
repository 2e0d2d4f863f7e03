"""Reward terms as fixed-shape arrays: why the team reward of the last step was what it was (include/cc4.h, cc4_reward_terms_device) -- which
subnet, which kind, whose Restore.  The step adds its reward up from a penalty per failed green action (LocalWork, AccessService), a penalty per
executed Impact and -1 per submitted Restore, and keeps only the sum; an env that records (enable_reward_terms(), or one that steps with red or
green actions) keeps the pieces of its last step.

Per subnet  [9, 4] int32   row s = the engine's subnet id (SUBNET_NAMES), columns TERM_COLUMNS: the three penalty sums (<= 0) and the number of
                           charged events, counted whatever their weight in this mission phase.
Words       [16] int32     WORDS: valid, step_count, phase, brm, action_cost, the five blue agents' shares (the terms of the subnets the agent
                           defends, ZONE_OF_SUBNET, plus its own Restore cost), the unowned rest, the five agents' own Restore costs.
'valid' is 1 iff the record was written by the step that produced the row; otherwise (a regenerated episode, a step taken without recording,
edit_state(SE_SET_STEP), no cold row) everything but step_count and phase is zero.  With valid set
    words[brm] + words[action_cost] == reward          and          sum(words[share_0 .. share_4]) + words[unowned] == words[brm] + words[action_cost]

Two ways to the same numbers:
  CC4VecEnv.reward_terms() / CC4TorchVecEnv.reward_terms()   the HIP kernel over the batch (k_reward_terms)
  from_row(hot, cold=None, steps=0)   the same definition compiled for the host (cc4_reward_terms_from_row): from cc4_get_state / cc4_get_cold
                                      rows or a checkpoint, in a process without a GPU"""
from . import _lib as L
from ._view_util import ZONE_OF_SUBNET, _rows, call_from_row  # noqa: F401  (ZONE_OF_SUBNET: part of this module's surface)

NUM_BLUE, SUBNETS, COLS, NWORDS = L.NUM_BLUE, L.REWARD_SUBNETS, L.REWARD_COLS, L.REWARD_WORDS

TERM_COLUMNS = {'lwf': 0, 'asf': 1, 'ria': 2, 'events': 3}
WORDS = {'valid': 0, 'step_count': 1, 'phase': 2, 'brm': 3, 'action_cost': 4,
         'share_0': 5, 'share_1': 6, 'share_2': 7, 'share_3': 8, 'share_4': 9, 'unowned': 10,
         'restore_0': 11, 'restore_1': 12, 'restore_2': 13, 'restore_3': 14, 'restore_4': 15}
SHARE_WORDS = slice(5, 10)               # words[..., SHARE_WORDS]: per blue agent
RESTORE_WORDS = slice(11, 16)
SUBNET_NAMES = ('restricted_zone_a_subnet', 'operational_zone_a_subnet', 'restricted_zone_b_subnet', 'operational_zone_b_subnet',
                'contractor_network_subnet', 'public_access_zone_subnet', 'admin_network_subnet', 'office_network_subnet',
                'internet_subnet')       # SUBNET enum order (wrappers.SUBNET_NAMES)


def from_row(hot, cold=None, steps=0):
    """(terms [9, 4] int32, words [16] int32) of one packed hot row (CC4VecEnv.get_state(e)) and its cold row (the second part of
    CC4VecEnv.snapshot(e)).  cold=None: valid is 0.  steps: the episode length of the env the rows come from; 0: the length the hot row itself
    records."""
    return call_from_row('reward_terms', *_rows(hot, cold), int(steps))[:2]       # (the record lies in the cold row's fixed part)
