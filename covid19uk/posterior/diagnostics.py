"""`python -m covid19uk.posterior.diagnostics` -- pools the diagnostics/ groups of chain files (the reference has no such tool)."""
from covid19uk_amd.posterior.diagnostics import *  # noqa: F401,F403
from covid19uk_amd.posterior.diagnostics import main  # noqa: F401

if __name__ == "__main__":
    main()
