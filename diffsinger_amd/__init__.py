"""diffsinger_amd - MI355X-native (gfx950) diffusion-denoiser hot path for DiffSinger / DiffSpeech.

Public surface mirrors the reference's own plugin API for this path:

    DIFF_DECODERS                       the registry the tasks index with hparams['diff_decoder_type']
                                        (usr/task.py:10, usr/diffspeech_task.py:12, usr/diffsinger_task.py:23)
    DiffNet(in_dims)                    usr/diff/net.py:81
    GaussianDiffusion(phone_encoder, out_dims, denoise_fn, timesteps, K_step, loss_type, betas, spec_min, spec_max)
                                        usr/diff/shallow_diffusion_tts.py:71  (+ .inference(cond, ...))
    register(*registries)               rebinds 'wavenet' (and adds 'wavenet_hip') in the reference's registries
    STFTLoss, MultiResolutionSTFTLoss   modules/parallel_wavegan/losses/stft_loss.py:76, :109 (+ the operators under them: stft_adjoint_op,
                                        spectral_loss_op; diffsinger_amd/stft_loss.py)
    ParallelWaveGANDiscriminator        modules/parallel_wavegan/models/parallel_wavegan.py:207, forward and backward on HIP (+ pwg_disc_op,
                                        lsgan_loss_op, generator_loss, discriminator_loss: modules/hifigan/hifigan.py:337-365;
                                        diffsinger_amd/pwg_disc.py)
    pwg_generator_losses, pwg_discriminator_losses, pwg_training_step
                                        the ParallelWaveGAN trainer's two objectives and one step of it (configs/tts/pwg.yaml) on
                                        ParallelWaveGANGenerator.forward_train (diffsinger_amd/pwg_train.py, + pwg_gen_op)
    avg_pool_op, cond_discriminator_loss
                                        MultiScaleDiscriminator's AvgPool1d(4, 2, 1) on HIP, forward and backward (modules/hifigan/hifigan.py:304)
                                        and hifigan.py:350-356 (diffsinger_amd/hifigan_disc.py)
    DiscriminatorP, MultiPeriodDiscriminator, disc_p_op, feature_loss, hifigan_adversarial_losses, hifigan_discriminator_losses
                                        the multi-period discriminator (modules/hifigan/hifigan.py:181-250), forward and backward on HIP, the
                                        feature-matching loss (:328-334) and the generator's / discriminator's terms against it
                                        (diffsinger_amd/hifigan_disc.py)
    DiscriminatorS, MultiScaleDiscriminator, disc_s_op
                                        the multi-scale discriminator (modules/hifigan/hifigan.py:253-325): the grouped strided Conv1d stack
                                        forward and backward on HIP, spectral and weight norm as torch expressions, the reference's state dict
                                        (diffsinger_amd/hifigan_disc.py)
    HifiGanMelLoss, mel_spectrogram_loss_op, spec_logmel_op
                                        the mel-spectrogram loss of the HiFi-GAN trainer (modules/hifigan/mel_utils.py:45-76, lambda_mel) on
                                        the differentiable log-mel (diffsinger_amd/mel_loss.py, diffsinger_amd/stft.py)
    hifigan_generator_losses, hifigan_generator_step, hifigan_training_step
                                        the mel term of the HiFi-GAN generator objective and one step on it, on
                                        HifiGanGenerator.forward_train; the full step with the adversarial and feature-matching terms
                                        against a list of discriminators, and their own objective (diffsinger_amd/hifigan_train.py)
    MultiTensorOptimizer, RAdam, AdamW, pwg_optimizers
                                        the vocoder rows' optimisers on HIP: one update over the list of parameter tensors with the
                                        global-norm clip folded in (clip_and_step); RAdam in the arithmetic of
                                        modules/parallel_wavegan/optimizers/radam.py, AdamW, and the RAdam + StepLR pairs of
                                        configs/tts/pwg.yaml (diffsinger_amd/voc_optim.py)
    pe_losses(output, sample, hp), pe_training_step(model, sample, hp)
                                        PitchExtractionTask.run_model / ._training_step (tasks/tts/pe.py:111-155) on the HIP PitchExtractor
                                        (diffsinger_amd/pe.py)

Importing the package does not load the HIP library; constructing an engine does, and fails loudly if
libdsdenoise.so is missing (no CPU fallback)."""
from .hparams import hparams, use_preset  # noqa: F401

__all__ = ['DIFF_DECODERS', 'DiffNet', 'GaussianDiffusion', 'OfflineGaussianDiffusion', 'register', 'hparams', 'use_preset',
           'STFTLoss', 'MultiResolutionSTFTLoss', 'stft_adjoint_op', 'spectral_loss_op',
           'ParallelWaveGANDiscriminator', 'pwg_disc_op', 'lsgan_loss_op', 'generator_loss', 'discriminator_loss',
           'pwg_gen_op', 'pwg_generator_losses', 'pwg_discriminator_losses', 'pwg_training_step',
           'avg_pool_op', 'cond_discriminator_loss',
           'DiscriminatorP', 'MultiPeriodDiscriminator', 'disc_p_op', 'feature_loss', 'hifigan_adversarial_losses', 'hifigan_discriminator_losses',
           'DiscriminatorS', 'MultiScaleDiscriminator', 'disc_s_op',
           'pe_losses', 'pe_training_step',
           'HifiGanMelLoss', 'mel_spectrogram_loss_op', 'spec_logmel_op', 'hifigan_generator_losses', 'hifigan_generator_step',
           'hifigan_training_step', 'MultiTensorOptimizer', 'RAdam', 'AdamW', 'pwg_optimizers']


def __getattr__(name):      # lazy: torch-heavy modules load on first use
    if name in ('DiffNet',):
        from .net import DiffNet
        return DiffNet
    if name in ('GaussianDiffusion', 'OfflineGaussianDiffusion'):
        from . import diffusion
        return getattr(diffusion, name)
    if name in ('DIFF_DECODERS', 'register'):
        from . import registry
        return getattr(registry, name)
    if name in ('STFTLoss', 'MultiResolutionSTFTLoss', 'stft_adjoint_op', 'spectral_loss_op'):
        from . import stft_loss
        return getattr(stft_loss, name)
    if name in ('ParallelWaveGANDiscriminator', 'pwg_disc_op', 'lsgan_loss_op', 'generator_loss', 'discriminator_loss'):
        from . import pwg_disc
        return getattr(pwg_disc, name)
    if name in ('pwg_gen_op', 'pwg_generator_losses', 'pwg_discriminator_losses', 'pwg_training_step'):
        from . import pwg_train
        return getattr(pwg_train, name)
    if name in ('avg_pool_op', 'cond_discriminator_loss', 'DiscriminatorP', 'MultiPeriodDiscriminator', 'disc_p_op', 'feature_loss',
                'hifigan_adversarial_losses', 'hifigan_discriminator_losses', 'DiscriminatorS', 'MultiScaleDiscriminator', 'disc_s_op'):
        from . import hifigan_disc
        return getattr(hifigan_disc, name)
    if name in ('pe_losses', 'pe_training_step'):
        from . import pe
        return getattr(pe, name)
    if name in ('HifiGanMelLoss', 'mel_spectrogram_loss_op'):
        from . import mel_loss
        return getattr(mel_loss, name)
    if name == 'spec_logmel_op':
        from .stft import spec_logmel_op
        return spec_logmel_op
    if name in ('hifigan_generator_losses', 'hifigan_generator_step', 'hifigan_training_step'):
        from . import hifigan_train
        return getattr(hifigan_train, name)
    if name in ('MultiTensorOptimizer', 'RAdam', 'AdamW', 'pwg_optimizers'):
        from . import voc_optim
        return getattr(voc_optim, name)
    raise AttributeError(name)
