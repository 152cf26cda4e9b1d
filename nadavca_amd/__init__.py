"""nadavca_amd — MI355X-native engine for Nadavca's signal-to-reference alignment path.

Public surface mirrors the reference package (/root/reference/nadavca/__init__.py:1-2):
``align_signal`` and ``estimate_snps``, plus the ``dtw`` operator module.  Importing the package
does not touch the GPU; every compute entry point goes through the HIP library
(nadavca_amd/csrc/libnadavca_hip.so) and fails loudly if it or the device is missing.
"""
from . import dtw  # noqa: F401
from .estimate_snps import estimate_snps, estimate_snps_batch  # noqa: F401
from .align_signal import align_signal, align_signal_batch  # noqa: F401
from .seedalign import SeedAligner  # noqa: F401
from .refset import ReferenceSet  # noqa: F401
from .kmer_train import estimate_kmer_model  # noqa: F401
from .call_mods import call_mods_batch  # noqa: F401
from .mod_train import ModModelEstimate, estimate_mod_model  # noqa: F401
from .call_indels import call_indels_batch  # noqa: F401
from .allele_fractions import estimate_allele_fractions_batch  # noqa: F401
from .phase import PhaseBatch, phase_reads_batch  # noqa: F401
from .phase_mods import PhasedModBatch, mod_site_frequencies, phase_mods_batch  # noqa: F401
from .site_levels import SiteComparison, SiteLevelBatch, compare_site_levels, site_levels_batch  # noqa: F401
from .site_ranks import SiteRankComparison, compare_site_ranks, site_rank_tests_batch  # noqa: F401
from .site_mixtures import SiteMixtureComparison, compare_site_mixtures, site_mixture_tests_batch  # noqa: F401
from .signal_map import SignalMapBatch, signal_map_batch  # noqa: F401
from .locate import LocateBatch, signal_locate_batch  # noqa: F401
from .decode import DecodeBatch, decode_batch  # noqa: F401
from .decode_fit import DecodeFit  # noqa: F401
from .decode_train import DecodeModelEstimate, estimate_decode_model  # noqa: F401
from .repeats import (RepeatCountBatch, RepeatItems, RepeatLocus, count_repeats_batch, repeat_chain,  # noqa: F401
                      repeat_items)

__all__ = ['align_signal', 'align_signal_batch', 'estimate_snps', 'estimate_snps_batch', 'dtw', 'SeedAligner',
           'ReferenceSet', 'estimate_kmer_model', 'call_mods_batch', 'call_indels_batch',
           'estimate_allele_fractions_batch', 'phase_reads_batch', 'PhaseBatch', 'phase_mods_batch', 'PhasedModBatch',
           'mod_site_frequencies', 'site_levels_batch',
           'compare_site_levels', 'SiteLevelBatch', 'SiteComparison', 'compare_site_ranks', 'site_rank_tests_batch', 'SiteRankComparison', 'compare_site_mixtures',
           'site_mixture_tests_batch', 'SiteMixtureComparison', 'estimate_mod_model', 'ModModelEstimate', 'signal_map_batch',
           'SignalMapBatch', 'signal_locate_batch', 'LocateBatch', 'decode_batch', 'DecodeBatch', 'DecodeFit',
           'estimate_decode_model', 'DecodeModelEstimate', 'count_repeats_batch', 'RepeatCountBatch', 'RepeatLocus',
           'RepeatItems', 'repeat_chain', 'repeat_items']
