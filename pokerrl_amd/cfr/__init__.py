from pokerrl_amd.cfr.DiscountedCFR import DiscountedCFR  # noqa: F401
