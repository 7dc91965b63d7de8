"""150 iterations of Discounted CFR (alpha, beta, gamma = 1.5, 0, 2) on DiscretizedNLLeduc, in the mould of run_lcfr_example.py."""
from _common import run

from pokerrl_amd.cfr.DiscountedCFR import DiscountedCFR

if __name__ == "__main__":
    run(DiscountedCFR, "DCFR_EXAMPLE")
