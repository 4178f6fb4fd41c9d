"""Region totals on the host: group specifications, group state, forecast planes and check counts
(covid19uk_amd/posterior/groups.py)."""
from covid19uk_amd.posterior.groups import *  # noqa: F401,F403
from covid19uk_amd.posterior.groups import GroupTable, parse_groups  # noqa: F401
