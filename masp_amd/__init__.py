"""masp_amd — MI355X-native Groth16 prover for the MASP Spend / Output / Convert circuits.

The compute path is the HIP library ``libmasp_hip.so`` (masp_amd/csrc, C ABI in include/masp_hip.h).
This package is the thin host side above that ABI; it contains no arithmetic fallback: if the
extension or a GPU is missing, calls raise.
"""
from .hip import Context, MaspHipError, library_path, load_library  # noqa: F401
from .r1cs import R1cs  # noqa: F401
from .verifier import (BatchValidator, Bundle, ConvertDescription, OutputDescription, SaplingVerificationContext,  # noqa: F401
                       SpendDescription)
from . import note_encryption  # noqa: F401
from .note_encryption import (CompactShieldedOutput, Note, PaymentAddress, Rseed, ShieldedOutput, note_nf, sapling_note_encrypt,  # noqa: F401
                              try_sapling_compact_note_decryption, try_sapling_note_decryption)
from . import redjubjub  # noqa: F401
from .redjubjub import sign_batch, spend_sigs  # noqa: F401
from . import merkle_tree  # noqa: F401
from .merkle_tree import CommitmentTree, FrozenCommitmentTree, IncrementalWitness, MerklePath, advance, empty_root  # noqa: F401
from . import convert  # noqa: F401
from .convert import AllowedConversion  # noqa: F401
