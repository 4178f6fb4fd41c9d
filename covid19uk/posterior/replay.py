"""`python -m covid19uk.posterior.replay` -- every product of the inference from finished posterior files."""
from covid19uk_amd.posterior.replay import *  # noqa: F401,F403
from covid19uk_amd.posterior.replay import main  # noqa: F401

if __name__ == "__main__":
    main()
