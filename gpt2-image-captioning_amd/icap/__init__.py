"""icap — MI355X-native (gfx950) prefix image-captioning hot path.

Drop-in for the device hot path of thenoobychocobo/gpt2-image-captioning
(src/models.py, src/train.py, src/embeddings/clip.py, src/embeddings/vit.py): all arithmetic runs in
the hand-written HIP kernels of libicap_hip.so (include/icap.h); PyTorch only
owns device memory, streams, graphs and torch.distributed.
"""

__version__ = "0.1.0"

from .clip import CLIPVisionConfig, CLIPVisionTower, extract_clip_embedding_from_image, extract_clip_embeddings, load_clip_model  # noqa: E402,F401
from .clip_text import (CLIPTextConfig, CLIPTextTower, ClipTextCore, chunk_captions,  # noqa: E402,F401
                        extract_caption_embeddings,
                        extract_clip_embedding_from_caption, get_image_id_from_filename, load_captions_annotations,
                        load_clip_text_model, load_image_embeddings_file_names, map_caption_id_to_caption)
from .jpeg import DeviceJpegDecoder, decode_jpeg, parse_jpeg  # noqa: E402,F401
from .dataset import CocoDataset, SyntheticCaptionDataset  # noqa: E402,F401
from .engine import CaptionScorer, CaptionTrainer  # noqa: E402,F401
from .gpt2 import GPT2Config, GPT2LMHeadModel  # noqa: E402,F401
from .mapper import MLPMappingNetwork, TransformerMappingNetwork  # noqa: E402,F401
from .models import (ImageCaptioningModel, RetrievalAggregator, RetrievalAugmentedTransformer,  # noqa: E402,F401
                     load_gpt2_tokenizer)
from .retrieval import (DeviceRetrievalStore, build_retrieval_store, create_retrieval_store,  # noqa: E402,F401
                        save_retrieval_store)
from .evaluate import evaluate_loss, evaluate_rat_epoch, generate_and_evaluate_rat  # noqa: E402,F401
from .metrics import DeviceCaptionMetrics  # noqa: E402,F401
from .train import train, train_rat  # noqa: E402,F401
from .vit import ViTConfig, ViTImageTower, extract_vit_embedding_from_image, extract_vit_embeddings, load_vit_model  # noqa: E402,F401
from .dino import (DINOv3ImageTower, DinoConfig, extract_dino_embeddings, get_dinov3_preprocessor,  # noqa: E402,F401
                   load_dinov3_models)
