"""Golden fixture for the image sheets: the reference's own recorded PNGs, decoded with Pillow and stored as uint8
arrays.  Data only: nothing of the reference's programs is run or copied.  Writes tests/golden/sheets_ref.npz (compressed).

    python tests/golden/make_golden_sheets.py <path of the reference repository> [output directory]

  countergan.original, .counterfactual, .delta [122][122][3]   conditional_counteRGAN/mnist/outputs3/{original,counterfactual,delta}.png:
                                                              save_image(..., nrow=4, normalize=True) of 16 images (gan_train.py:161-163)
  mnist_gan.epoch1 [152][152][3]                              simple_gan/mnist/output/images/1.png: save_image(generated_images.data[:25],
                                                              nrow=5, normalize=True) (mnist_gan.py:141)"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = {"countergan.original": "conditional_counteRGAN/mnist/outputs3/original.png",
         "countergan.counterfactual": "conditional_counteRGAN/mnist/outputs3/counterfactual.png",
         "countergan.delta": "conditional_counteRGAN/mnist/outputs3/delta.png",
         "mnist_gan.epoch1": "simple_gan/mnist/output/images/1.png"}


def main(ref, out_dir=HERE):
    arrays = {}
    for key, rel in FILES.items():
        with Image.open(os.path.join(ref, rel)) as im:
            assert im.mode == "RGB", (rel, im.mode)
            arrays[key] = np.asarray(im, dtype=np.uint8).copy()
        print(key, arrays[key].shape)
    np.savez_compressed(os.path.join(out_dir, "sheets_ref.npz"), **arrays)


if __name__ == "__main__":
    main(*sys.argv[1:3])
