"""Build the MI355X HIP extension in-tree.

    python setup.py build_ext --inplace

Cross-compiles for gfx950 via hipcc (no GPU needed to build). The resulting
_smxgb_hip.so lives inside the package so it travels with the source tree.
"""
import os

from setuptools import find_packages, setup

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")
os.environ.setdefault("MAX_JOBS", "8")

from torch.utils.cpp_extension import BuildExtension, CUDAExtension  # noqa: E402


class BuildExt(BuildExtension):
    """The ninja rule for hipcc records no header dependencies, so an edit
    to a shared header would leave stale objects behind. Objects older than
    the newest header in `depends` are dropped before the build and ninja
    compiles them again."""

    def build_extension(self, ext):
        headers = [h for h in ext.depends if os.path.exists(h)]
        if headers and os.path.isdir(self.build_temp):
            newest = max(os.path.getmtime(h) for h in headers)
            for root, _, files in os.walk(self.build_temp):
                for name in files:
                    path = os.path.join(root, name)
                    if name.endswith(".o") and os.path.getmtime(path) < newest:
                        os.remove(path)
        super().build_extension(ext)


setup(
    name="sagemaker_xgboost_container_amd",
    version="0.1.0",
    description="MI355X-native SageMaker XGBoost training/serving framework",
    packages=find_packages(exclude=("tests",)),
    ext_modules=[
        CUDAExtension(
            name="sagemaker_xgboost_container_amd.ops._smxgb_hip",
            sources=[
                "sagemaker_xgboost_container_amd/ops/csrc/smxgb_kernels.hip",
                "sagemaker_xgboost_container_amd/ops/csrc/smxgb_sparse.hip",
                "sagemaker_xgboost_container_amd/ops/csrc/smxgb_shap_compact.hip",
                "sagemaker_xgboost_container_amd/ops/csrc/smxgb_sampling.hip",
                "sagemaker_xgboost_container_amd/ops/csrc/smxgb_quantile.hip",
                "sagemaker_xgboost_container_amd/ops/csrc/text_parsers.cpp",
            ],
            # headers shared by the sources: a change rebuilds the extension
            depends=[
                "sagemaker_xgboost_container_amd/ops/csrc/smxgb_cat.h",
                "sagemaker_xgboost_container_amd/ops/csrc/smxgb_jobs.h",
                "sagemaker_xgboost_container_amd/ops/csrc/smxgb_shap.h",
            ],
            extra_compile_args={
                "cxx": ["-O3"],
                "nvcc": ["-O3", "--offload-arch=gfx950"],
            },
        )
    ],
    cmdclass={"build_ext": BuildExt},
    entry_points={
        "console_scripts": [
            "serve = sagemaker_xgboost_container_amd.serving:serving_entrypoint",
        ]
    },
)
