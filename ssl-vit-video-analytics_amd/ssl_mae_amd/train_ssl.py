"""`python -m ssl_mae_amd.train_ssl --config configs/ssl_train.yaml`: the reference's module
name (src/train_ssl.py) for ssl_mae_amd.temporal_ssl."""
from .temporal_ssl import (TemporalSSL, _perm_index_4way, build_mask, cosine_loss, main,  # noqa: F401
                           permute_frames_4way, train_one_epoch, update_ema, variance_loss)

if __name__ == "__main__":
    main()
